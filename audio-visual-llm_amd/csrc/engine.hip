// Model-level entry points: the kernel sequences for the Whisper encoder, the CLIP vision tower, and the
// Llama + LoRA forward / backward / KV-cache decode.  Host-side C++ only enqueues kernels on the caller's
// stream (no allocation, no sync), so a caller can capture any of these into a hipGraph.
//
// Reference call stacks: encode_audio clip_whisper_model.py:1067-1106 -> WhisperEncoder.forward
// HF:models/whisper/modeling_whisper.py:592-646; encode_video :1108-1146 -> CLIPVisionModel.forward
// HF:models/clip/modeling_clip.py:641-656; self.llm(...) :602-613 -> LlamaForCausalLM.forward
// HF:models/llama/modeling_llama.py:435-488; loss.backward() trainer/clip_whisper_trainer.py:454.
#include "common.h"
#include "avllm_internal.h"

namespace {

struct Bump {
    char* base; size_t cap; size_t off = 0; bool ok = true;
    Bump(void* p, size_t c) : base((char*)p), cap(c) {}
    void* take(size_t bytes) {
        const size_t a = (off + 255) & ~(size_t)255;
        if (a + bytes > cap) { ok = false; off = a + bytes; return base; }
        off = a + bytes;
        return base + a;
    }
};
// dry-run sizing uses a null base and an unlimited cap
inline size_t bump_size(const Bump& b) { return ((b.off + 255) & ~(size_t)255) + 256; }

inline avllm_gemm_desc gemm_desc(int dtype, const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K) {
    avllm_gemm_desc g = {};
    g.A = A; g.B = B; g.C = C; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.dtype = dtype; g.alpha = 1.0f;
    return g;
}

inline AvRopeScale llama_rope_scale(const avllm_llama* m) {
    AvRopeScale sc;
    sc.factor = m->rope_factor; sc.low_freq_factor = m->rope_low_freq_factor; sc.high_freq_factor = m->rope_high_freq_factor; sc.orig_ctx = m->rope_orig_ctx;
    return sc;
}

// ------------------------------------------------------------------ block-scaled fp8 projections (BASELINE config 5)
// Scratch for the quantised activation of one projection input: codes [M, Kmax] + its scale image.  One quantisation serves every
// projection that reads the same input (q, k and v of a decoder layer).
struct F8Buf { void* q = nullptr; void* s = nullptr; };
void carve_f8(Bump& b, F8Buf& f, long M, int kmax) {
    f.q = b.take((size_t)M * kmax);
    f.s = b.take(avllm_mx_scale_bytes((int)M, kmax));
}
inline int f8_quant(const F8Buf& f, const void* x, long ldx, int M, int K, hipStream_t st) {
    return av_mx_quantize(x, ldx, M, K, f.q, K, f.s, 0, AV_BF16, st);
}
// C = act(Aq.W8^T + bias) + R with the activation already quantised into f
inline int f8_proj(const F8Buf& f, int M, int K, const void* W8, const void* S8, int N, void* C, long ldc, const void* bias, int act, const void* R,
                   long ldr, hipStream_t st) {
    avllm_gemm_f8_desc d = {};
    d.A = f.q; d.SA = f.s; d.B = W8; d.SB = S8; d.C = C; d.bias = bias; d.R = R;
    d.lda = K; d.ldb = K; d.ldc = ldc; d.ldr = ldr; d.M = M; d.N = N; d.K = K; d.act = act;
    return av_gemm_f8(&d, st);
}

// One frozen linear layer, y = act(x W^T + bias) + R, on the matrix in the mode's form.  f8 == nullptr: W in the activation dtype (av_gemm).
// Otherwise the e4m3 image W8 with its scales S8 times the block-scaled codes of x in *f8; x is quantised here unless the caller says the
// codes are already there (after av_norm_mxq, after av_attention_fwd_mxq, for a second projection of the same input).
struct Frozen { const void *W, *W8, *S8, *bias; };
int linear(int dtype, const F8Buf* f8, bool quantised, const Frozen& w, const void* x, long ldx, int M, int K, int N, void* y, long ldy, int act,
           const void* R, long ldr, hipStream_t st) {
    if (f8) {
        if (!quantised) AV_TRY(f8_quant(*f8, x, ldx, M, K, st));
        return f8_proj(*f8, M, K, w.W8, w.S8, N, y, ldy, w.bias, act, R, ldr, st);
    }
    avllm_gemm_desc g = gemm_desc(dtype, x, ldx, w.W, K, y, ldy, M, N, K);
    g.bias = w.bias; g.act = act; g.R = R; g.ldr = ldr;
    return av_gemm(&g, st);
}

// ------------------------------------------------------------------ encoders
// xc / xcn: the CLS rows of the last block (CLIP only)
struct EncBuf { void *x, *xn, *qkv, *att, *ff, *xc, *xcn; F8Buf f8; };
void carve_enc(Bump& b, EncBuf& e, long M, long cls_rows, int d, int ffn, size_t es, bool fp8) {
    e.x = b.take((size_t)M * d * es);
    e.xn = b.take((size_t)M * d * es);
    e.qkv = b.take((size_t)M * 3 * d * es);
    e.att = b.take((size_t)M * d * es);
    e.ff = b.take((size_t)M * ffn * es);
    if (cls_rows) {
        e.xc = b.take((size_t)cls_rows * d * es);
        e.xcn = b.take((size_t)cls_rows * d * es);
    }
    if (fp8) carve_f8(b, e.f8, M, ffn > d ? ffn : d);
}

int encoder_layers(int dtype, const avllm_enc_layer* L, int layers, int d, int heads, int ffn, int tokens, long items,
                   float eps, int act, const EncBuf& b, bool cls_only_last, void* cls_out, hipStream_t st, bool fp8 = false) {
    const long M = items * tokens;
    const int hd = d / heads;
    const size_t es = av_dtype_size(dtype);
    for (int l = 0; l < layers; ++l) {
        const avllm_enc_layer& P = L[l];
        AV_CHECK_ARG(!fp8 || (P.wqkv8 && P.sqkv8 && P.wo8 && P.so8 && P.w18 && P.s18 && P.w28 && P.s28), "encoder layer %d: fp8 mode without fp8 weight images", l);
        const F8Buf* fq = fp8 ? &b.f8 : nullptr;
        const bool nq = fp8 && d % 128 == 0 && d <= 8192 && !av_knob(AV_KNOB_F8_UNFUSED_QUANT);      // LayerNorm straight to e4m3 + scales (fp8.hip norm_mxq_kernel)
        if (nq) AV_TRY(av_norm_mxq(b.x, P.ln1_w, P.ln1_b, nullptr, nullptr, b.f8.q, d, b.f8.s, M, d, eps, st));
        else AV_TRY(av_layernorm(b.x, P.ln1_w, P.ln1_b, b.xn, M, d, eps, dtype, st));
        AV_TRY(linear(dtype, fq, nq, {P.wqkv, P.wqkv8, P.sqkv8, P.bqkv}, b.xn, d, (int)M, d, 3 * d, b.qkv, 3 * d, AV_ACT_NONE, nullptr, 0, st));
        const char* qkv = (const char*)b.qkv;
        // only token 0 of the last block is consumed (clip_whisper_model.py:1141): the block is finished on the CLS rows, a handful, in the
        // activation dtype also in fp8 mode
        const bool cls = cls_only_last && l == layers - 1;
        // fp8: the attention output is only ever the out-projection's A operand -- the one-pass kernel (CLIP: <= 272 tokens) block-scales it in its
        // epilogue; the bf16 tensor is not written (the CLS-only last block keeps the bf16 form)
        const bool att_q = fp8 && !cls && av_attention_fwd_mxq_ok((int)items, tokens, heads, hd, dtype, heads);
        if (att_q) AV_TRY(av_attention_fwd_mxq(qkv, qkv + (size_t)d * es, qkv + (size_t)2 * d * es, b.f8.q, d, b.f8.s, (int)items, tokens, heads, hd,
                                               3 * d, 3 * d, 3 * d, 1.0f / sqrtf((float)hd), st));
        else
        AV_TRY(av_attention_fwd(qkv, qkv + (size_t)d * es, qkv + (size_t)2 * d * es, b.att, nullptr, (int)items, tokens, tokens,
                                heads, hd, 3 * d, 3 * d, 3 * d, d, 1.0f / sqrtf((float)hd), 0, dtype, 0, st));
        // the block tail: rows of the token-major buffers (row stride d), or their CLS rows (stride tokens * d) into xc -> xcn -> cls_out
        if (cls) fq = nullptr;
        const int rows = cls ? (int)items : (int)M;
        const long ldx = cls ? (long)tokens * d : d;
        void* x1 = cls ? b.xc : b.x;
        void* xn = cls ? b.xcn : b.xn;
        void* out = cls ? cls_out : b.x;
        AV_TRY(linear(dtype, fq, att_q, {P.wo, P.wo8, P.so8, P.bo}, b.att, ldx, rows, d, d, x1, d, AV_ACT_NONE, b.x, ldx, st));
        const bool nq2 = nq && !cls;
        if (nq2) AV_TRY(av_norm_mxq(x1, P.ln2_w, P.ln2_b, nullptr, nullptr, b.f8.q, d, b.f8.s, rows, d, eps, st));
        else AV_TRY(av_layernorm(x1, P.ln2_w, P.ln2_b, xn, rows, d, eps, dtype, st));
        if (fq) {
            if (!nq2) AV_TRY(f8_quant(*fq, xn, d, rows, d, st));      // fc1's input: in the F8Buf from here on, either way
            // fc1 with its output quantised in the epilogue (codes + scale image live in the bf16 ff buffer's memory: 1 + 1/32 of its 2 bytes
            // per element), so fc2 reads them directly: no bf16 copy of the [M, ffn] activation, no quantiser pass over it
            avllm_gemm_f8_desc q1 = {};
            q1.A = b.f8.q; q1.SA = b.f8.s; q1.B = P.w18; q1.SB = P.s18; q1.bias = P.b1; q1.lda = d; q1.ldb = d; q1.M = rows; q1.N = ffn; q1.K = d; q1.act = act;
            F8Buf ffq;
            ffq.q = b.ff; ffq.s = (char*)b.ff + (((size_t)M * ffn + 255) & ~(size_t)255);
            q1.Cq = ffq.q; q1.SCq = ffq.s; q1.ldcq = ffn;
            if (!av_knob(AV_KNOB_F8_UNFUSED_QUANT) && avllm_gemm_f8_takes_quantised_output(&q1) && (size_t)M * ffn + 256 + avllm_mx_scale_bytes((int)M, ffn) <= (size_t)M * ffn * es) {
                AV_TRY(av_gemm_f8(&q1, st));
                AV_TRY(linear(dtype, &ffq, true, {P.w2, P.w28, P.s28, P.b2}, b.ff, ffn, rows, ffn, d, out, d, AV_ACT_NONE, x1, d, st));
                continue;
            }
        }
        AV_TRY(linear(dtype, fq, true, {P.w1, P.w18, P.s18, P.b1}, xn, d, rows, d, ffn, b.ff, ffn, act, nullptr, 0, st));
        AV_TRY(linear(dtype, fq, false, {P.w2, P.w28, P.s28, P.b2}, b.ff, ffn, rows, ffn, d, out, d, AV_ACT_NONE, x1, d, st));
    }
    return AV_OK;
}

struct WhisperWs { void *cols1, *h1, *cols2; EncBuf e; };
void carve_whisper(const avllm_whisper* w, int B, Bump& b, WhisperWs& s) {
    const size_t es = av_dtype_size(w->dtype);
    const long T2 = 2L * w->n_ctx, M = (long)B * w->n_ctx;
    s.cols1 = b.take((size_t)B * T2 * w->k1pad * es);
    s.h1 = b.take((size_t)B * T2 * w->d * es);
    s.cols2 = b.take((size_t)M * 3 * w->d * es);
    carve_enc(b, s.e, M, 0, w->d, w->ffn, es, w->fp8 != 0);
}

struct ClipWs { void* cols; EncBuf e; };
void carve_clip(const avllm_clip* c, int N, Bump& b, ClipWs& s, int& kpad) {
    const size_t es = av_dtype_size(c->dtype);
    const int g = c->image / c->patch;
    kpad = (3 * c->patch * c->patch + 63) / 64 * 64;
    s.cols = b.take((size_t)N * g * g * kpad * es);
    carve_enc(b, s.e, (long)N * c->tokens, N, c->d, c->ffn, es, c->fp8 != 0);
}

// ------------------------------------------------------------------ llama
// grouped-query geometry: q is d wide, k and v are dkv = kv_heads*hd wide; the fused row is [q | k | v] = qw columns
inline int llama_kv_heads(const avllm_llama* m) { return m->kv_heads > 0 ? m->kv_heads : m->heads; }
inline int llama_dkv(const avllm_llama* m) { return llama_kv_heads(m) * (m->d / m->heads); }
inline int llama_qw(const avllm_llama* m) { return m->d + 2 * llama_dkv(m); }
inline int llama_off(const avllm_llama* m, int j) { return j == 0 ? 0 : (j == 1 ? m->d : m->d + llama_dkv(m)); }     // column (= wqkv row) of slice j
inline int llama_wid(const avllm_llama* m, int j) { return j == 0 ? m->d : llama_dkv(m); }
// slice j of a layer's q|k|v bias (NULL without one)
inline const void* llama_bias(const avllm_llama* m, const avllm_llama_layer& P, int j) {
    return P.bqkv ? (const char*)P.bqkv + (size_t)llama_off(m, j) * av_dtype_size(m->dtype) : nullptr;
}

// label smoothing or z-loss in the training objective: either value non-zero takes the av_ce_smooth pair, both 0 exactly av_ce_fwd / av_ce_bwd
inline bool llama_loss_smooth(const avllm_loss_opts* o) { return o && (o->label_smoothing != 0.f || o->z_loss != 0.f); }
// per-head q/k RMSNorm (Qwen3): a model has it on every layer or on none (check_llama)
inline bool llama_qk_norm(const avllm_llama* m) { return m->layer && m->layer[0].q_norm_w != nullptr; }
// adapters on gate_proj / up_proj / down_proj (avllm_llama_layer.lora_mlp): k = 0 gate, 1 up, 2 down
inline bool layer_mlp_lora(const avllm_llama_layer& P) { return P.lora_mlp[0].A_pad || P.lora_mlp[1].A_pad || P.lora_mlp[2].A_pad; }
inline bool llama_mlp_lora(const avllm_llama* m, int k0 = 0, int k1 = 3) {
    if (!m->layer) return false;
    for (int l = 0; l < m->layers; ++l)
        for (int k = k0; k < k1; ++k)
            if (m->layer[l].lora_mlp[k].A_pad) return true;
    return false;
}
// the kernels that read an adapter's [M, K] input can generate its dropout mask themselves (lora_drop below)
inline bool lora_mask_fusable(const avllm_llama* m, int K) { return m->dtype == AV_BF16 && K % 256 == 0 && m->lora_r <= 16; }

struct LlamaLayerAct {
    void *xn1, *qkv, *att, *tqkv, *to, *h1, *gu;
    float *rstd1, *rstd2, *lse;
    void* qk_pre; float* qk_rstd;      // q/k head norm only: the pre-norm q|k [M, d + dkv] and rstd [M, H + Hkv] for avllm_qk_norm_bwd
    void *tgu, *tdown;                 // MLP adapters only: the rank-side products of gate | up [M, 2*64] and of down [M, 64]
};
struct LlamaTrainWs {
    void** resid;            // host array [layers+1]
    LlamaLayerAct* act;      // host array [layers]
    void *xn2, *hmid, *xf, *logits, *xd;
    float *rstd_f, *row_lse, *delta, *rope_tab;
    // backward scratch
    void *dres, *dxn, *dgu, *dhmid, *dqkv, *datt, *dtqkv, *dto;
    F8Buf f8;                // fp8 mode: the quantised input of the projection being computed
    void *dtgu, *dtdown;     // MLP adapters only: the gradients of tgu / tdown
    void* xdf;               //   and dropout(hmid) [M, ffn] where down's mask is materialised (lora_mask_fusable fails for K = ffn)
};

void carve_llama_train(const avllm_llama* m, int B, int S, Bump& b, LlamaTrainWs& w, void** resid, LlamaLayerAct* act) {
    const size_t es = av_dtype_size(m->dtype);
    const long M = (long)B * S;
    const int d = m->d, f = m->ffn;
    w.resid = resid; w.act = act;
    for (int l = 0; l <= m->layers; ++l) resid[l] = b.take((size_t)M * d * es);
    for (int l = 0; l < m->layers; ++l) {
        LlamaLayerAct& a = act[l];
        a.xn1 = b.take((size_t)M * d * es);
        a.qkv = b.take((size_t)M * llama_qw(m) * es);
        a.att = b.take((size_t)M * d * es);
        a.tqkv = b.take((size_t)M * 3 * AVLLM_LORA_PAD * es);
        a.to = b.take((size_t)M * AVLLM_LORA_PAD * es);
        a.h1 = b.take((size_t)M * d * es);
        a.gu = b.take((size_t)M * 2 * f * es);
        a.rstd1 = (float*)b.take((size_t)M * 4);
        a.rstd2 = (float*)b.take((size_t)M * 4);
        a.lse = (float*)b.take((size_t)B * m->heads * S * 4);
    }
    w.xn2 = b.take((size_t)M * d * es);
    w.hmid = b.take((size_t)M * f * es);
    w.xf = b.take((size_t)M * d * es);
    w.logits = b.take((size_t)M * m->vocab * es);
    w.xd = b.take((size_t)M * d * es);
    w.rstd_f = (float*)b.take((size_t)M * 4);
    w.row_lse = (float*)b.take((size_t)M * 4);
    w.delta = (float*)b.take((size_t)B * m->heads * S * 4);
    w.rope_tab = (float*)b.take((size_t)S * (d / m->heads) * 4);
    w.dres = b.take((size_t)M * d * es);
    w.dxn = b.take((size_t)M * d * es);
    w.dgu = b.take((size_t)M * 2 * f * es);
    w.dhmid = b.take((size_t)M * f * es);
    w.dqkv = b.take((size_t)M * llama_qw(m) * es);
    w.datt = b.take((size_t)M * d * es);
    w.dtqkv = b.take((size_t)M * 3 * AVLLM_LORA_PAD * es);
    w.dto = b.take((size_t)M * AVLLM_LORA_PAD * es);
    if (m->fp8) carve_f8(b, w.f8, M, f > d ? f : d);
    // after everything else, and only for a model that has the head norms: every other model's layout and size stay what they were
    for (int l = 0; l < m->layers; ++l) {
        act[l].qk_pre = nullptr; act[l].qk_rstd = nullptr;
        if (!llama_qk_norm(m)) continue;
        act[l].qk_pre = b.take((size_t)M * (d + llama_dkv(m)) * es);
        act[l].qk_rstd = (float*)b.take((size_t)M * (m->heads + llama_kv_heads(m)) * 4);
    }
    // the same rule for a model with an adapter on gate, up or down
    w.dtgu = w.dtdown = w.xdf = nullptr;
    const bool mlp = llama_mlp_lora(m);
    for (int l = 0; l < m->layers; ++l) {
        act[l].tgu = act[l].tdown = nullptr;
        if (!mlp) continue;
        act[l].tgu = b.take((size_t)M * 2 * AVLLM_LORA_PAD * es);
        act[l].tdown = b.take((size_t)M * AVLLM_LORA_PAD * es);
    }
    if (mlp) {
        w.dtgu = b.take((size_t)M * 2 * AVLLM_LORA_PAD * es);
        w.dtdown = b.take((size_t)M * AVLLM_LORA_PAD * es);
        if (llama_mlp_lora(m, 2, 3) && !lora_mask_fusable(m, f)) w.xdf = b.take((size_t)M * f * es);
    }
}
// The training workspace laid out in ws (null with an unlimited size: the dry run that sizes it), with the host arrays its layout points into
struct LlamaTrainFrame {
    Bump b; LlamaTrainWs w; void* resid[257]; LlamaLayerAct act[256];
    LlamaTrainFrame(const avllm_llama* m, int B, int S, void* ws, size_t ws_bytes) : b(ws, ws_bytes) { carve_llama_train(m, B, S, b, w, resid, act); }
};

int check_llama(const avllm_llama* m) {
    AV_CHECK_ARG(m && m->layer && m->embed && m->norm_w && m->lm_head, "llama: null model fields");
    AV_CHECK_ARG(m->d % m->heads == 0 && m->d % 64 == 0 && m->ffn % 64 == 0, "llama: d=%d ffn=%d must be multiples of 64", m->d, m->ffn);
    AV_CHECK_ARG(m->layers > 0 && m->layers <= 256, "llama: layers=%d", m->layers);
    AV_CHECK_ARG(m->kv_heads >= 0 && (m->kv_heads == 0 || m->heads % m->kv_heads == 0), "llama: heads=%d kv_heads=%d", m->heads, m->kv_heads);
    for (int l = 0; l < m->layers; ++l) {
        const avllm_llama_layer& P = m->layer[l];
        AV_CHECK_ARG((P.q_norm_w != nullptr) == (P.k_norm_w != nullptr) && (P.q_norm_w != nullptr) == llama_qk_norm(m),
                     "llama layer %d: q_norm_w and k_norm_w go together, on every layer or on none", l);
    }
    AV_CHECK_ARG(!llama_qk_norm(m) || m->d / m->heads == 64 || m->d / m->heads == 128, "llama: q/k head norms need a head dim of 64 or 128 (%d)", m->d / m->heads);
    AV_CHECK_ARG(!m->fp8 || !llama_mlp_lora(m), "llama: fp8 mode does not take adapters on gate_proj / up_proj / down_proj (lora_mlp)");
    if (m->fp8)
        for (int l = 0; l < m->layers; ++l) {
            const avllm_llama_layer& P = m->layer[l];
            AV_CHECK_ARG(P.wqkv8 && P.sqkv8 && P.wo8 && P.so8 && P.wgu8 && P.sgu8 && P.wdown8 && P.sdown8, "llama layer %d: fp8 mode without fp8 weight images", l);
        }
    if (m->decode_fp8 || m->decode_fp4) {
        AV_CHECK_ARG(!(m->decode_fp8 && m->decode_fp4), "llama: decode_fp4 and decode_fp8 are two forms of the same token step, set one");
        const bool f4 = m->decode_fp4 != 0;
        const char* mode = f4 ? "decode_fp4" : "decode_fp8";
        AV_CHECK_ARG(m->dtype == AV_BF16 && m->d % 128 == 0 && m->ffn % 128 == 0 && m->vocab % 16 == 0 && m->lm_head8 && m->elm_head8,
                     "llama: %s needs bf16, d and ffn multiples of 128, vocab a multiple of 16 and the e4m3 lm_head codes + exponents", mode);
        for (int l = 0; l < m->layers; ++l) {
            const avllm_llama_layer& P = m->layer[l];
            AV_CHECK_ARG(f4 ? P.wqkv4 && P.eqkv4 && P.wo4 && P.eo4 && P.wgu4 && P.egu4 && P.wdown4 && P.edown4
                            : P.wqkv8 && P.eqkv8 && P.wo8 && P.eo8 && P.wgu8 && P.egu8 && P.wdown8 && P.edown8,
                         "llama layer %d: %s without the %s codes and their exponents", l, mode, f4 ? "MXFP4" : "fp8");
        }
    }
    return AV_OK;
}

// ------------------------------------------------------------------ LoRA adapters
// The step's adapter dropout (peft: lora_B(lora_A(dropout(x))), one mask per wrapped module).  p = 0: none.  fused: the kernels that read the
// adapter's input generate its mask themselves (bf16 MFMA kernels); otherwise (fp32 parity mode, narrow models) dropout(x) is materialised.
// The backward pass regenerates the forward's masks from the same seeds, so both take this rule from here.
struct LoraDrop {
    float p; bool fused;
    float fused_p() const { return fused ? p : 0.f; }
};
// K: the input width of the modules meant (d; ffn for down_proj).  The mask index of an element is row * K + col.
inline LoraDrop lora_drop(const avllm_llama* m, int K) {
    const float p = m->lora_dropout > 0.f ? m->lora_dropout : 0.f;
    return {p, p > 0.f && lora_mask_fusable(m, K)};
}
inline LoraDrop lora_drop(const avllm_llama* m) { return lora_drop(m, m->d); }
// the mask of layer l, module j (q, k, v, o; then 4 gate, 5 up, 6 down, whose seeds follow those of all layers' attention modules: the
// attention seeds stay what they were).  The step's base seed may live in device memory instead (m->dropout_seed_dev, see avllm_step_state)
inline uint32_t lora_seed(const avllm_llama* m, int l, int j) {
    return j < 4 ? m->dropout_seed + 4u * l + j : m->dropout_seed + 4u * m->layers + 3u * l + (j - 4);
}
// the adapter branch's input: x [M, K] itself, or dropout(x) in xd after an av_dropout launch when masks are materialised
int lora_input(const avllm_llama* m, const LoraDrop& dr, const void* x, void* xd, int M, int K, uint32_t seed, const void*& xl, hipStream_t st) {
    xl = x;
    if (dr.p > 0.f && !dr.fused) {
        AV_CHECK_ARG(xd, "llama: no dropout buffer for an adapter input of width %d", K);
        AV_TRY(av_dropout(x, xd, M, K, seed, dr.p, m->dtype, st, m->dropout_seed_dev));
        xl = xd;
    }
    return AV_OK;
}

// Adapter j of layer l in the training workspace: q, k, v (j = 0..2) share the [M, 3*64] buffers tqkv / dtqkv, o (j = 3) has to / dto,
// gate and up (j = 4, 5) share the [M, 2*64] buffers tgu / dtgu, down (j = 6) has tdown / dtdown
struct LoraView {
    const avllm_lora_mod* mod;
    uint32_t seed;
    void *t, *dt; long ldt;      // forward t_j = s dropout_j(x) A_j^T, backward d t_j, and the row stride of both
    int off, wid;                // its columns of the fused q|k|v (gate|up) row (o, down: its own d columns)
    bool at_slice;               // AT_pad is the j-th 64-column slice of one [d, 3*64] matrix that starts at q's (gate, up: [d, 2*64], gate's)
    int K;                       // width of its input: d, or ffn for down
};
inline LoraView lora_view(const avllm_llama* m, int l, int j, const LlamaLayerAct& a, const LlamaTrainWs& w) {
    const avllm_lora_mod* lora = m->layer[l].lora;
    const size_t es_ = av_dtype_size(m->dtype);
    if (j >= 4) {
        const avllm_lora_mod* lm = m->layer[l].lora_mlp;
        const int k = j - 4;
        if (k == 2) return {&lm[2], lora_seed(m, l, j), a.tdown, w.dtdown, AVLLM_LORA_PAD, 0, m->d, false, m->ffn};
        const size_t slot = (size_t)k * AVLLM_LORA_PAD * es_;
        LoraView g = {&lm[k], lora_seed(m, l, j), a.tgu ? (char*)a.tgu + slot : nullptr, w.dtgu ? (char*)w.dtgu + slot : nullptr, 2 * AVLLM_LORA_PAD,
                      k * m->ffn, m->ffn, false, m->d};
        g.at_slice = lm[k].ld_at == 2 * AVLLM_LORA_PAD && (const char*)lm[k].AT_pad == (const char*)lm[0].AT_pad + slot;
        return g;
    }
    LoraView v = {&lora[j], lora_seed(m, l, j), a.to, w.dto, AVLLM_LORA_PAD, 0, m->d, false, m->d};
    if (j < 3) {
        const size_t es = av_dtype_size(m->dtype), slot = (size_t)j * AVLLM_LORA_PAD * es;
        v.t = (char*)a.tqkv + slot; v.dt = (char*)w.dtqkv + slot; v.ldt = 3 * AVLLM_LORA_PAD;
        v.off = llama_off(m, j); v.wid = llama_wid(m, j);
        v.at_slice = lora[j].ld_at == 3 * AVLLM_LORA_PAD && (const char*)lora[j].AT_pad == (const char*)lora[0].AT_pad + slot;
    }
    return v;
}

// One adapted projection of x [M, K]: y = x W^T + bias + R + t B^T with t = s * dropout(x) A^T, the rank-side product of xl (lora_input),
// made here unless have_t.  W is the frozen matrix for the base product with the adapter as its second K segment (bf16 / fp32); W == nullptr
// (fp8 mode) means y already holds the base product with its bias and residual, and the adapter term is added by a K = 64 GEMM.
int lora_linear(const avllm_llama* m, const void* x, int K, const void* W, const void* bias, int N, const avllm_lora_mod& lm, const void* xl,
                uint32_t a_seed, float a_p, void* t, long ldt, bool have_t, void* y, long ldy, const void* R, long ldr, int M, hipStream_t st) {
    avllm_gemm_desc g;
    const bool has = lm.A_pad != nullptr;
    if (has && !have_t) {
        g = gemm_desc(m->dtype, xl, K, lm.A_pad, K, t, ldt, M, AVLLM_LORA_PAD, K);
        g.alpha = m->lora_scale;
        g.a_drop_seed = a_seed; g.a_drop_p = a_p; g.seed_dev = m->dropout_seed_dev;      // bf16: dropout generated inside the rank-side GEMM
        g.n_valid = m->lora_r;                         // rank padded to 64: the padding columns are written as zeros, not computed
        AV_TRY(av_gemm(&g, st));
    }
    if (W) {
        g = gemm_desc(m->dtype, x, K, W, K, y, ldy, M, N, K);
        if (has) { g.A2 = t; g.lda2 = ldt; g.B2 = lm.B_pad; g.ldb2 = AVLLM_LORA_PAD; g.K2 = AVLLM_LORA_PAD; }
        g.R = R; g.ldr = ldr; g.bias = bias;
    } else {
        if (!has) return AV_OK;
        g = gemm_desc(m->dtype, t, ldt, lm.B_pad, AVLLM_LORA_PAD, y, ldy, M, N, AVLLM_LORA_PAD);
        g.R = y; g.ldr = ldy;
    }
    return av_gemm(&g, st);
}

// One adapter's weight gradients and d t from dy, its columns of the projection's output gradient: dB += dy^T t, dt = s dy B,
// dA += dt^T dropout(x)
int lora_wgrad(const avllm_llama* m, const LoraDrop& dr, const LoraView& v, const void* dy, long ldy, const void* x, void* xd, int M, hipStream_t st) {
    const avllm_lora_mod& lm = *v.mod;
    const int dt = m->dtype, d = v.K, R = m->lora_r;
    AV_TRY(av_gemm_tn(dy, ldy, v.wid, v.t, v.ldt, R, M, lm.gB, R, 1.0f, dt, st));
    avllm_gemm_desc gt = gemm_desc(dt, dy, ldy, lm.BT_pad, v.wid, v.dt, v.ldt, M, AVLLM_LORA_PAD, v.wid);
    gt.alpha = m->lora_scale; gt.n_valid = R;
    AV_TRY(av_gemm(&gt, st));
    const void* xin;
    AV_TRY(lora_input(m, dr, x, xd, M, d, v.seed, xin, st));
    return av_gemm_tn(v.dt, v.ldt, R, xin, d, d, M, lm.gA, d, 1.0f, dt, st, v.seed, dr.fused_p(), m->dropout_seed_dev);
}

// dx += sum_j mask_j * (dt_j . A_j) / (1-p) over the adapters present among v[0..n): their input gradients pass back through their dropout.
// One pass over dx for all of them when the fused kernel applies (csrc/lora_dx.hip), a masked K = 64 GEMM each otherwise (p = 0: a plain
// accumulating one, for adapters whose AT images are not the slices of one matrix).  dx is [M, d_in], d_in the adapters' input width.
int lora_dx_dropped(const avllm_llama* m, const LoraDrop& dr, const LoraView* v, int n, void* dx, int M, hipStream_t st, int d_in = 0) {
    const int dt = m->dtype, d = d_in ? d_in : m->d;
    const void* Tp[3]; const void* Ap[3]; long lt[3], la[3]; uint32_t sd[3]; int nj = 0;
    for (int j = 0; j < n; ++j) {
        if (!v[j].mod->A_pad) continue;
        Tp[nj] = v[j].dt; lt[nj] = v[j].ldt; Ap[nj] = v[j].mod->AT_pad; la[nj] = v[j].mod->ld_at; sd[nj] = v[j].seed; ++nj;
    }
    if (dr.fused && av_lora_dx_masked_supported(dt, d, m->lora_r, lt, la, nj, d, d))
        return av_lora_dx_masked(Tp, lt, Ap, la, sd, nj, m->lora_r, dx, d, dx, d, M, d, dr.p, m->dropout_seed_dev, dt, st);
    for (int k = 0; k < nj; ++k) {
        avllm_gemm_desc gm = gemm_desc(dt, Tp[k], lt[k], Ap[k], la[k], dx, d, M, d, AVLLM_LORA_PAD);
        gm.R = dx; gm.ldr = d; gm.drop_seed = sd[k]; gm.drop_p = dr.p; gm.seed_dev = m->dropout_seed_dev;
        AV_TRY(av_gemm(&gm, st));
    }
    return AV_OK;
}

// The MLP half of one layer's backward pass when the layer has an adapter on gate, up or down: from dres = d resid[l+1] to dxn = d xn2
// (the caller's post-attention RMSNorm backward follows).  `gd` is the caller's dhmid = dres Wdown_t product, not yet launched.
// The workspace keeps one xn2 and one hmid for all layers, so both adapter inputs are made again: xn2 by the forward's norm kernel from the
// saved h1, hmid by the SwiGLU backward itself (av_swiglu_bwd_h), which therefore runs before dA_down.
int llama_mlp_lora_bwd(const avllm_llama* m, int l, LlamaTrainWs& w, avllm_gemm_desc gd, int M, hipStream_t st) {
    const avllm_llama_layer& P = m->layer[l];
    LlamaLayerAct& a = w.act[l];
    const int dt = m->dtype, d = m->d, f = m->ffn, R = m->lora_r;
    const size_t es = av_dtype_size(dt);
    const LoraDrop dr = lora_drop(m), drf = lora_drop(m, f);
    const bool drop = dr.p > 0.f;
    const LoraView vm[3] = {lora_view(m, l, 4, a, w), lora_view(m, l, 5, a, w), lora_view(m, l, 6, a, w)};
    // ---- down: resid[l+1] = h1 + hmid Wdown^T + t_down B_down^T;  dy = dres
    const bool down = vm[2].mod->A_pad != nullptr;
    if (down) {
        const avllm_lora_mod& lm = *vm[2].mod;
        AV_TRY(av_gemm_tn(w.dres, d, d, vm[2].t, vm[2].ldt, R, M, lm.gB, R, 1.0f, dt, st));                         // dB = dy^T t
        avllm_gemm_desc gt = gemm_desc(dt, w.dres, d, lm.BT_pad, d, vm[2].dt, vm[2].ldt, M, AVLLM_LORA_PAD, d);   // dt = s dy B
        gt.alpha = m->lora_scale; gt.n_valid = R;
        AV_TRY(av_gemm(&gt, st));
        if (!drop) { gd.A2 = vm[2].dt; gd.lda2 = vm[2].ldt; gd.B2 = lm.AT_pad; gd.ldb2 = lm.ld_at; gd.K2 = AVLLM_LORA_PAD; }
    }
    AV_TRY(av_gemm(&gd, st));
    if (down && drop) AV_TRY(lora_dx_dropped(m, drf, &vm[2], 1, w.dhmid, M, st, f));
    if (down) {
        AV_TRY(av_swiglu_bwd_h(w.dhmid, a.gu, w.dgu, w.hmid, M, f, dt, st));
        const void* xin;
        AV_TRY(lora_input(m, drf, w.hmid, w.xdf, M, f, vm[2].seed, xin, st));
        AV_TRY(av_gemm_tn(vm[2].dt, vm[2].ldt, R, xin, f, f, M, vm[2].mod->gA, f, 1.0f, dt, st, vm[2].seed, drf.fused_p(), m->dropout_seed_dev));   // dA = dt^T dropout(hmid)
    } else AV_TRY(av_swiglu_bwd(w.dhmid, a.gu, w.dgu, M, f, dt, st));
    // ---- gate, up: gu = xn2 Wgu^T + [t_gate B_gate^T | t_up B_up^T];  dy_k = the k-th column half of dgu
    const bool gate = vm[0].mod->A_pad != nullptr, up = vm[1].mod->A_pad != nullptr, any = gate || up;
    char* dgu = (char*)w.dgu;
    if (any) AV_TRY(av_rmsnorm_fwd(a.h1, P.ln2_w, w.xn2, nullptr, M, d, m->eps, dt, st));
    const bool batch = dt == AV_BF16 && gate && up && (!drop || dr.fused) && d % 256 == 0 && f % 256 == 0 && av_lora_batch_supported(dt, R, 2) &&
                       !av_knob(AV_KNOB_LORA_UNBATCHED);
    if (batch) {      // three launches for the two adapters' dB, dt and dA (csrc/lora_batch.hip) instead of six
        const void* Tq[2]; long ldt2[2]; float* gBp[2]; long lgb[2]; int c0[2], nc[2];
        const void* dyp[2]; long ldy[2]; const void* BTp[2]; long lbt[2]; void* dtp[2];
        const void* dtc[2]; float* gAp[2]; long lga[2]; uint32_t sd[2];
        for (int k = 0; k < 2; ++k) {
            const avllm_lora_mod& lk = *vm[k].mod;
            Tq[k] = vm[k].t; dtp[k] = vm[k].dt; dtc[k] = vm[k].dt; ldt2[k] = vm[k].ldt; sd[k] = vm[k].seed;
            c0[k] = vm[k].off; nc[k] = f; lbt[k] = f;
            dyp[k] = dgu + (size_t)vm[k].off * es; ldy[k] = 2 * f; BTp[k] = lk.BT_pad;
            gBp[k] = lk.gB; lgb[k] = R; gAp[k] = lk.gA; lga[k] = d;
        }
        AV_TRY(av_gemm_tn_multi(dgu, 2 * f, 2 * f, Tq, ldt2, gBp, lgb, c0, nc, nullptr, 2, R, M, 1.0f, 0.f, nullptr, 0, dt, st));
        AV_TRY(av_lora_rank3(dyp, ldy, nc, BTp, lbt, dtp, ldt2, nullptr, 2, M, R, m->lora_scale, 0.f, nullptr, 0, dt, st));
        AV_TRY(av_gemm_tn_multi(w.xn2, d, d, dtc, ldt2, gAp, lga, nullptr, nullptr, sd, 2, R, M, 1.0f, dr.p, m->dropout_seed_dev, 1, dt, st));
    } else
    for (int k = 0; k < 2; ++k)
        if (vm[k].mod->A_pad) AV_TRY(lora_wgrad(m, dr, vm[k], dgu + (size_t)vm[k].off * es, 2 * f, w.xn2, w.xd, M, st));
    // both adapters as one [d,128] AT image ride in the frozen product; one alone, or with dropout, adds its term afterwards
    const bool seg = gate && up && !drop && vm[0].at_slice && vm[1].at_slice;
    avllm_gemm_desc g = gemm_desc(dt, w.dgu, 2 * f, P.wgu_t, 2 * f, w.dxn, d, M, d, 2 * f);
    if (seg) { g.A2 = w.dtgu; g.lda2 = 2 * AVLLM_LORA_PAD; g.B2 = vm[0].mod->AT_pad; g.ldb2 = 2 * AVLLM_LORA_PAD; g.K2 = 2 * AVLLM_LORA_PAD; }
    AV_TRY(av_gemm(&g, st));
    if (any && !seg) AV_TRY(lora_dx_dropped(m, dr, vm, 2, w.dxn, M, st));
    return AV_OK;
}

}  // namespace

// =============================================================================================== Whisper
extern "C" size_t avllm_whisper_workspace_bytes(const avllm_whisper* w, int32_t B) {
    Bump b(nullptr, (size_t)-1);
    WhisperWs s;
    carve_whisper(w, B, b, s);
    return bump_size(b);
}

extern "C" int avllm_whisper_encoder_fwd(const avllm_whisper* w, const float* mel, int32_t B, void* out, void* ws,
                                         size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AV_CHECK_ARG(w && mel && out && ws && B > 0, "whisper_encoder_fwd: null/empty");
    AV_CHECK_ARG(w->d % w->heads == 0 && w->d % 64 == 0 && w->ffn % 64 == 0 && w->k1pad % 64 == 0 && w->k1pad >= 3 * w->n_mels,
                 "whisper: d=%d ffn=%d k1pad=%d unsupported", w->d, w->ffn, w->k1pad);
    Bump b(ws, ws_bytes);
    WhisperWs s;
    carve_whisper(w, B, b, s);
    if (!b.ok) return av_set_error(AV_ERR_WORKSPACE, "whisper_encoder_fwd: workspace %zu < %zu bytes", ws_bytes, bump_size(b));
    const int dt = w->dtype, d = w->d, T2 = 2 * w->n_ctx;
    const long M = (long)B * w->n_ctx;
    AV_TRY(av_whisper_im2col1(mel, s.cols1, B, w->n_mels, T2, w->k1pad, dt, st));
    avllm_gemm_desc g = gemm_desc(dt, s.cols1, w->k1pad, w->conv1_w, w->k1pad, s.h1, d, B * T2, d, w->k1pad);
    g.bias = w->conv1_b; g.act = AV_ACT_GELU;
    AV_TRY(av_gemm(&g, st));
    AV_TRY(av_whisper_im2col2(s.h1, s.cols2, B, T2, d, dt, st));
    g = gemm_desc(dt, s.cols2, 3 * d, w->conv2_w, 3 * d, s.e.x, d, (int)M, d, 3 * d);
    g.bias = w->conv2_b; g.act = AV_ACT_GELU; g.R = w->pos; g.ldr = d; g.r_mod = w->n_ctx;
    AV_TRY(av_gemm(&g, st));
    AV_CHECK_ARG(!w->fp8 || (dt == AV_BF16 && d % 128 == 0 && w->ffn % 128 == 0), "whisper: fp8 needs bf16 activations and widths that are multiples of 128");
    AV_TRY(encoder_layers(dt, w->layer, w->layers, d, w->heads, w->ffn, w->n_ctx, B, 1e-5f, AV_ACT_GELU, s.e, false, nullptr,
                          st, w->fp8 != 0));
    return av_layernorm(s.e.x, w->lnf_w, w->lnf_b, out, M, d, 1e-5f, dt, st);
}

// =============================================================================================== CLIP
extern "C" size_t avllm_clip_workspace_bytes(const avllm_clip* c, int32_t N) {
    Bump b(nullptr, (size_t)-1);
    ClipWs s; int kpad;
    carve_clip(c, N, b, s, kpad);
    return bump_size(b);
}

extern "C" int avllm_clip_vision_cls_fwd(const avllm_clip* c, const void* frames, int32_t N, void* cls, void* ws,
                                         size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AV_CHECK_ARG(c && frames && cls && ws && N > 0, "clip_vision_cls_fwd: null/empty");
    // the CLS rows reach `cls` through the last block's tail alone: without a block nothing would write it
    AV_CHECK_ARG(c->layers >= 1 && c->layer, "clip_vision_cls_fwd: layers=%d: the output is written by the last block, a tower without one has none", c->layers);
    const int g1 = c->image / c->patch;
    AV_CHECK_ARG(c->tokens == g1 * g1 + 1 && c->d % c->heads == 0 && c->d % 64 == 0 && c->ffn % 64 == 0,
                 "clip: tokens=%d d=%d ffn=%d inconsistent", c->tokens, c->d, c->ffn);
    Bump b(ws, ws_bytes);
    ClipWs s; int kpad;
    carve_clip(c, N, b, s, kpad);
    if (!b.ok) return av_set_error(AV_ERR_WORKSPACE, "clip_vision_cls_fwd: workspace %zu < %zu bytes", ws_bytes, bump_size(b));
    const int dt = c->dtype, d = c->d, np = g1 * g1;
    const size_t es = av_dtype_size(dt);
    AV_TRY(av_clip_patchify(frames, s.cols, N, c->image, c->patch, kpad, dt, st, c->frames_bf16 ? AV_BF16 : AV_F32));
    // patch embedding + position embedding of the patch tokens, scattered to rows 1.. of each frame
    avllm_gemm_desc g = gemm_desc(dt, s.cols, kpad, c->patch_w, kpad, s.e.xn, d, N * np, d, kpad);
    g.R = (const char*)c->pos + (size_t)d * es; g.ldr = d; g.r_mod = np;
    g.g_in = np; g.g_out = c->tokens; g.g_off = 1;
    AV_TRY(av_gemm(&g, st));
    AV_TRY(av_clip_cls_rows(c->class_emb, c->pos, s.e.xn, N, c->tokens, d, dt, st));
    AV_TRY(av_layernorm(s.e.xn, c->pre_ln_w, c->pre_ln_b, s.e.x, (long)N * c->tokens, d, c->eps, dt, st));
    AV_CHECK_ARG(!c->fp8 || (dt == AV_BF16 && d % 128 == 0 && c->ffn % 128 == 0), "clip: fp8 needs bf16 activations and widths that are multiples of 128");
    return encoder_layers(dt, c->layer, c->layers, d, c->heads, c->ffn, c->tokens, N, c->eps, AV_ACT_QUICK_GELU, s.e, true, cls,
                          st, c->fp8 != 0);
}

// =============================================================================================== Llama train
extern "C" size_t avllm_llama_train_workspace_bytes(const avllm_llama* m, int32_t B, int32_t S) {
    if (!m || m->layers > 256) return 0;
    return bump_size(LlamaTrainFrame(m, B, S, nullptr, (size_t)-1).b);
}

extern "C" int avllm_llama_lora_fwd_loss(const avllm_llama* m, const void* x, const int64_t* labels, int32_t B, int32_t S,
                                         void* logits_out, float* loss_sum, float* count, void* ws, size_t ws_bytes, void* stream) {
    return avllm_llama_lora_fwd_loss_opts(m, x, labels, B, S, logits_out, loss_sum, count, nullptr, ws, ws_bytes, stream);
}

extern "C" int avllm_llama_lora_fwd_loss_opts(const avllm_llama* m, const void* x, const int64_t* labels, int32_t B, int32_t S, void* logits_out,
                                              float* loss_sum, float* count, const avllm_loss_opts* opts, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AV_TRY(check_llama(m));
    AV_CHECK_ARG(x && ws && B > 0 && S > 0, "llama_lora_fwd_loss: null/empty");
    AV_CHECK_ARG(!labels || (loss_sum && count), "llama_lora_fwd_loss: labels need loss_sum/count");
    LlamaTrainFrame fr(m, B, S, ws, ws_bytes);
    if (!fr.b.ok) return av_set_error(AV_ERR_WORKSPACE, "llama_lora_fwd_loss: workspace %zu < %zu bytes", ws_bytes, bump_size(fr.b));
    LlamaTrainWs& w = fr.w;
    const int dt = m->dtype, d = m->d, f = m->ffn, H = m->heads, hd = d / H;
    const int Hkv = llama_kv_heads(m), dkv = llama_dkv(m), qw = llama_qw(m);
    const size_t es = av_dtype_size(dt);
    const int M = B * S;
    AV_HIP(hipMemcpyAsync(w.resid[0], x, (size_t)M * d * es, hipMemcpyDeviceToDevice, st));
    AV_TRY(av_rope_table(w.rope_tab, S, hd, 0, m->theta, st, nullptr, llama_rope_scale(m)));
    const LoraDrop dr = lora_drop(m);
    AV_CHECK_ARG(!m->fp8 || (dt == AV_BF16 && d % 128 == 0 && f % 128 == 0 && m->vocab % 8 == 0 && m->lm_head8 && m->slm_head8),
                 "llama: fp8 needs bf16 activations, d and ffn multiples of 128 and the fp8 weight images");
    const F8Buf* fq = m->fp8 ? &w.f8 : nullptr;      // fp8 mode: frozen products on the e4m3 images, the adapters' terms added on top in bf16
    for (int l = 0; l < m->layers; ++l) {
        const avllm_llama_layer& P = m->layer[l];
        LlamaLayerAct& a = w.act[l];
        const LoraView v[4] = {lora_view(m, l, 0, a, w), lora_view(m, l, 1, a, w), lora_view(m, l, 2, a, w), lora_view(m, l, 3, a, w)};
        AV_TRY(av_rmsnorm_fwd(w.resid[l], P.ln1_w, a.xn1, a.rstd1, M, d, m->eps, dt, st));
        // fp8: one product for q|k|v (one quantisation of the normed input)
        if (fq) AV_TRY(linear(dt, fq, false, {nullptr, P.wqkv8, P.sqkv8, P.bqkv}, a.xn1, d, M, d, qw, a.qkv, qw, AV_ACT_NONE, nullptr, 0, st));
        // all three rank-side products t_j = s * dropout_j(xn1) A_j^T in one launch (xn1 read once): csrc/lora_batch.hip
        const bool batch_qkv = !fq && dt == AV_BF16 && P.lora[0].A_pad && P.lora[1].A_pad && P.lora[2].A_pad && (dr.p == 0.f || dr.fused) &&
                               d % 256 == 0 && av_lora_batch_supported(dt, m->lora_r, 3) && !av_knob(AV_KNOB_LORA_UNBATCHED);
        if (batch_qkv) {
            const void* Ap[3] = {a.xn1, a.xn1, a.xn1}; const long la[3] = {d, d, d}; const int Kk[3] = {d, d, d};
            const void* Bp[3] = {P.lora[0].A_pad, P.lora[1].A_pad, P.lora[2].A_pad}; const long lb[3] = {d, d, d};
            void* Cp[3]; long lc[3]; uint32_t sd[3];
            for (int j = 0; j < 3; ++j) { Cp[j] = v[j].t; lc[j] = v[j].ldt; sd[j] = v[j].seed; }
            AV_TRY(av_lora_rank3(Ap, la, Kk, Bp, lb, Cp, lc, sd, 3, M, m->lora_r, m->lora_scale, dr.p, m->dropout_seed_dev, 1, dt, st));
        }
        for (int j = 0; j < 3; ++j) {
            const void* xl = a.xn1;
            if (v[j].mod->A_pad) AV_TRY(lora_input(m, dr, a.xn1, w.xd, M, d, v[j].seed, xl, st));
            AV_TRY(lora_linear(m, a.xn1, d, fq ? nullptr : (const char*)P.wqkv + (size_t)v[j].off * d * es, llama_bias(m, P, j), v[j].wid, *v[j].mod,
                               xl, v[j].seed, dr.fused_p(), v[j].t, v[j].ldt, batch_qkv, (char*)a.qkv + (size_t)v[j].off * es, qw, nullptr, 0, M, st));
        }
        // q and k slices are adjacent: H + Hkv heads.  With head norms the one pass normalises, rotates and saves what its backward reads.
        if (P.q_norm_w) AV_TRY(av_qk_norm_rope(a.qkv, qw, M, S, H, Hkv, hd, P.q_norm_w, P.k_norm_w, m->eps, w.rope_tab, a.qk_pre, a.qk_rstd, nullptr,
                                               nullptr, 0, 0, nullptr, dt, st));
        else AV_TRY(av_rope_tab(a.qkv, qw, M, S, H + Hkv, hd, w.rope_tab, 0, dt, st));
        const char* qkv = (const char*)a.qkv;
        AV_TRY(av_attention_fwd(qkv, qkv + (size_t)d * es, qkv + (size_t)(d + dkv) * es, a.att, a.lse, B, S, S, H, hd, qw, qw,
                                qw, d, 1.0f / sqrtf((float)hd), 1, dt, 0, st, Hkv));
        const void* xl = a.att;
        if (v[3].mod->A_pad) AV_TRY(lora_input(m, dr, a.att, w.xd, M, d, v[3].seed, xl, st));
        if (fq) AV_TRY(linear(dt, fq, false, {nullptr, P.wo8, P.so8, P.bo}, a.att, d, M, d, d, a.h1, d, AV_ACT_NONE, w.resid[l], d, st));
        AV_TRY(lora_linear(m, a.att, d, fq ? nullptr : P.wo, P.bo, d, *v[3].mod, xl, v[3].seed, dr.fused_p(), v[3].t, v[3].ldt, false, a.h1, d,
                           w.resid[l], d, M, st));
        AV_TRY(av_rmsnorm_fwd(a.h1, P.ln2_w, w.xn2, a.rstd2, M, d, m->eps, dt, st));
        if (!layer_mlp_lora(P)) {      // the frozen MLP: exactly the launches of a model without MLP adapters
            AV_TRY(linear(dt, fq, false, {P.wgu, P.wgu8, P.sgu8, nullptr}, w.xn2, d, M, d, 2 * f, a.gu, 2 * f, AV_ACT_NONE, nullptr, 0, st));
            AV_TRY(av_swiglu_fwd(a.gu, w.hmid, M, f, dt, st));
            AV_TRY(linear(dt, fq, false, {P.wdown, P.wdown8, P.sdown8, nullptr}, w.hmid, f, M, f, d, w.resid[l + 1], d, AV_ACT_NONE, a.h1, d, st));
            continue;
        }
        // ---- MLP with adapters: gu = xn2 Wgu^T + [t_gate B_gate^T | t_up B_up^T], resid[l+1] = h1 + hmid Wdown^T + t_down B_down^T.  gate and
        // up are the row halves of wgu and the column halves of gu: two N = f products, each with its adapter as second K segment
        const LoraView vm[3] = {lora_view(m, l, 4, a, w), lora_view(m, l, 5, a, w), lora_view(m, l, 6, a, w)};
        const bool batch_gu = dt == AV_BF16 && vm[0].mod->A_pad && vm[1].mod->A_pad && (dr.p == 0.f || dr.fused) && d % 256 == 0 &&
                              av_lora_batch_supported(dt, m->lora_r, 2) && !av_knob(AV_KNOB_LORA_UNBATCHED);
        if (batch_gu) {      // both rank-side products of xn2 in one launch
            const void* Ap[2] = {w.xn2, w.xn2}; const long la[2] = {d, d}; const int Kk[2] = {d, d};
            const void* Bp[2] = {vm[0].mod->A_pad, vm[1].mod->A_pad}; const long lb[2] = {d, d};
            void* Cp[2] = {vm[0].t, vm[1].t}; const long lc[2] = {vm[0].ldt, vm[1].ldt}; const uint32_t sd[2] = {vm[0].seed, vm[1].seed};
            AV_TRY(av_lora_rank3(Ap, la, Kk, Bp, lb, Cp, lc, sd, 2, M, m->lora_r, m->lora_scale, dr.p, m->dropout_seed_dev, 1, dt, st));
        }
        for (int k = 0; k < 2; ++k) {
            const void* xg = w.xn2;
            if (vm[k].mod->A_pad) AV_TRY(lora_input(m, dr, w.xn2, w.xd, M, d, vm[k].seed, xg, st));
            AV_TRY(lora_linear(m, w.xn2, d, (const char*)P.wgu + (size_t)vm[k].off * d * es, nullptr, f, *vm[k].mod, xg, vm[k].seed, dr.fused_p(), vm[k].t,
                               vm[k].ldt, batch_gu, (char*)a.gu + (size_t)vm[k].off * es, 2 * f, nullptr, 0, M, st));
        }
        AV_TRY(av_swiglu_fwd(a.gu, w.hmid, M, f, dt, st));
        const LoraDrop drf = lora_drop(m, f);      // down's input is ffn wide: its own fused-mask condition and mask index
        const void* xdn = w.hmid;
        if (vm[2].mod->A_pad) AV_TRY(lora_input(m, drf, w.hmid, w.xdf, M, f, vm[2].seed, xdn, st));
        AV_TRY(lora_linear(m, w.hmid, f, P.wdown, nullptr, d, *vm[2].mod, xdn, vm[2].seed, drf.fused_p(), vm[2].t, vm[2].ldt, false, w.resid[l + 1], d,
                           a.h1, d, M, st));
    }
    AV_TRY(av_rmsnorm_fwd(w.resid[m->layers], m->norm_w, w.xf, w.rstd_f, M, d, m->eps, dt, st));
    AV_TRY(linear(dt, fq, false, {m->lm_head, m->lm_head8, m->slm_head8, nullptr}, w.xf, d, M, d, m->vocab, w.logits, m->vocab, AV_ACT_NONE, nullptr, 0, st));
    if (logits_out) AV_HIP(hipMemcpyAsync(logits_out, w.logits, (size_t)M * m->vocab * es, hipMemcpyDeviceToDevice, st));
    if (labels) {
        if (llama_loss_smooth(opts))      // label smoothing / z-loss: the one-pass kernel that also gathers the row's sum of logits
            AV_TRY(av_ce_smooth_fwd(w.logits, m->vocab, labels, B, S, m->vocab, opts->label_smoothing, opts->z_loss, w.row_lse, loss_sum, count, opts->loss_terms, dt, st));
        else AV_TRY(av_ce_fwd(w.logits, m->vocab, labels, B, S, m->vocab, w.row_lse, loss_sum, count, dt, st));
    }
    return AV_OK;
}

extern "C" int avllm_llama_lora_bwd(const avllm_llama* m, const int64_t* labels, int32_t B, int32_t S, const float* count,
                                    float grad_scale, void* ws, size_t ws_bytes, avllm_layer_cb after_layer, void* user,
                                    void* stream) {
    AV_TRY(check_llama(m));
    return avllm_llama_lora_bwd_layers(m, labels, B, S, count, grad_scale, ws, ws_bytes, m->layers - 1, 0, after_layer, user, stream);
}

extern "C" int avllm_llama_lora_bwd_layers(const avllm_llama* m, const int64_t* labels, int32_t B, int32_t S, const float* count,
                                           float grad_scale, void* ws, size_t ws_bytes, int32_t layer_hi, int32_t layer_lo,
                                           avllm_layer_cb after_layer, void* user, void* stream) {
    return avllm_llama_lora_bwd_layers_dx(m, labels, B, S, count, grad_scale, ws, ws_bytes, layer_hi, layer_lo, after_layer, user, nullptr, stream);
}

extern "C" int avllm_llama_lora_bwd_layers_dx(const avllm_llama* m, const int64_t* labels, int32_t B, int32_t S, const float* count,
                                              float grad_scale, void* ws, size_t ws_bytes, int32_t layer_hi, int32_t layer_lo,
                                              avllm_layer_cb after_layer, void* user, void* dx_embeds, void* stream) {
    return avllm_llama_lora_bwd_layers_dx_opts(m, labels, B, S, count, grad_scale, ws, ws_bytes, layer_hi, layer_lo, after_layer, user, dx_embeds, nullptr, stream);
}

extern "C" int avllm_llama_lora_bwd_layers_dx_opts(const avllm_llama* m, const int64_t* labels, int32_t B, int32_t S, const float* count,
                                                   float grad_scale, void* ws, size_t ws_bytes, int32_t layer_hi, int32_t layer_lo,
                                                   avllm_layer_cb after_layer, void* user, void* dx_embeds, const avllm_loss_opts* opts, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AV_TRY(check_llama(m));
    AV_CHECK_ARG(layer_lo >= 0 && layer_lo <= layer_hi && layer_hi < m->layers, "llama_lora_bwd_layers: bad layer range [%d, %d]", layer_lo, layer_hi);
    AV_CHECK_ARG(labels && count && ws && m->lm_head_t, "llama_lora_bwd: null (training needs the transposed weight images)");
    LlamaTrainFrame fr(m, B, S, ws, ws_bytes);
    if (!fr.b.ok) return av_set_error(AV_ERR_WORKSPACE, "llama_lora_bwd: workspace %zu < %zu bytes", ws_bytes, bump_size(fr.b));
    LlamaTrainWs& w = fr.w;
    const int dt = m->dtype, d = m->d, f = m->ffn, H = m->heads, hd = d / H, V = m->vocab;
    const int Hkv = llama_kv_heads(m), dkv = llama_dkv(m), qw = llama_qw(m);
    const size_t es = av_dtype_size(dt);
    const int M = B * S, R = m->lora_r;
    const LoraDrop dr = lora_drop(m);      // the forward's rule and seeds: the masks are regenerated, not stored
    const bool drop = dr.p > 0.f;
    avllm_gemm_desc g;
    if (layer_hi == m->layers - 1) {      // the piece that starts at the top also runs loss -> lm_head -> final norm
        if (llama_loss_smooth(opts)) AV_TRY(av_ce_smooth_bwd(w.logits, V, labels, w.row_lse, count, grad_scale, opts->label_smoothing, opts->z_loss, w.logits, B, S, V, dt, st));
        else AV_TRY(av_ce_bwd(w.logits, V, labels, w.row_lse, count, grad_scale, w.logits, B, S, V, dt, st));
        g = gemm_desc(dt, w.logits, V, m->lm_head_t, V, w.dxn, d, M, d, V);
        AV_CHECK_ARG(V % 64 == 0, "llama_lora_bwd: vocab %d must be a multiple of 64", V);
        AV_TRY(av_gemm(&g, st));
        AV_TRY(av_rmsnorm_bwd(w.dxn, w.resid[m->layers], m->norm_w, w.rstd_f, nullptr, w.dres, M, d, dt, st));
    }
    for (int l = layer_hi; l >= layer_lo; --l) {
        const avllm_llama_layer& P = m->layer[l];
        LlamaLayerAct& a = w.act[l];
        const LoraView v[4] = {lora_view(m, l, 0, a, w), lora_view(m, l, 1, a, w), lora_view(m, l, 2, a, w), lora_view(m, l, 3, a, w)};
        AV_CHECK_ARG(P.wqkv_t && P.wo_t && P.wgu_t && P.wdown_t, "llama_lora_bwd: layer %d has no transposed weights", l);
        // ---- MLP: resid[l+1] = h1 + down(silu(g)*u)
        g = gemm_desc(dt, w.dres, d, P.wdown_t, d, w.dhmid, f, M, f, d);
        if (!layer_mlp_lora(P)) {      // the frozen MLP: exactly the launches of a model without MLP adapters
            AV_TRY(av_gemm(&g, st));
            AV_TRY(av_swiglu_bwd(w.dhmid, a.gu, w.dgu, M, f, dt, st));
            g = gemm_desc(dt, w.dgu, 2 * f, P.wgu_t, 2 * f, w.dxn, d, M, d, 2 * f);
            AV_TRY(av_gemm(&g, st));
        } else AV_TRY(llama_mlp_lora_bwd(m, l, w, g, M, st));
        AV_TRY(av_rmsnorm_bwd(w.dxn, a.h1, P.ln2_w, a.rstd2, w.dres, w.dres, M, d, dt, st));      // dres = d h1
        // ---- o_proj (+LoRA): h1 = resid[l] + att Wo^T + to Bo^T
        const avllm_lora_mod& lo = *v[3].mod;
        g = gemm_desc(dt, w.dres, d, P.wo_t, d, w.datt, d, M, d, d);
        if (lo.A_pad) {
            AV_TRY(lora_wgrad(m, dr, v[3], w.dres, d, a.att, w.xd, M, st));
            // without dropout the adapter's input gradient rides in the frozen product as its second K segment
            if (!drop) { g.A2 = v[3].dt; g.lda2 = v[3].ldt; g.B2 = lo.AT_pad; g.ldb2 = lo.ld_at; g.K2 = AVLLM_LORA_PAD; }
        }
        AV_TRY(av_gemm(&g, st));
        if (lo.A_pad && drop) AV_TRY(lora_dx_dropped(m, dr, &v[3], 1, w.datt, M, st));
        // ---- attention
        const char* qkv = (const char*)a.qkv;
        char* dqkv = (char*)w.dqkv;
        const bool fuse_rope = av_attention_bwd_fuses_rope(dt, hd, 0);      // bf16: the inverse RoPE rides in the dq/dk epilogues
        AV_TRY(av_attention_bwd(qkv, qkv + (size_t)d * es, qkv + (size_t)(d + dkv) * es, a.att, w.datt, a.lse, dqkv, dqkv + (size_t)d * es,
                                dqkv + (size_t)(d + dkv) * es, w.delta, B, S, H, hd, qw, qw, qw, d, qw, qw, qw,
                                1.0f / sqrtf((float)hd), 1, dt, 0, st, Hkv, fuse_rope ? w.rope_tab : nullptr));
        if (!fuse_rope) AV_TRY(av_rope_tab(dqkv, qw, M, S, H + Hkv, hd, w.rope_tab, 1, dt, st));
        // dqkv's q and k slices now hold the gradient of the normed pre-RoPE heads: through the head norm, before any projection gradient reads it
        if (P.q_norm_w) AV_TRY(av_qk_norm_bwd(dqkv, qw, M, H, Hkv, hd, P.q_norm_w, P.k_norm_w, a.qk_pre, a.qk_rstd, dt, st));
        // ---- q,k,v projections (+LoRA)
        bool any = false, contiguous = true;      // contiguous: all three present, their AT_pad images the slices of one [d,192] matrix
        for (int j = 0; j < 3; ++j) { any |= v[j].mod->A_pad != nullptr; contiguous &= v[j].mod->A_pad && v[j].at_slice; }
        const bool batch_bwd = dt == AV_BF16 && P.lora[0].A_pad && P.lora[1].A_pad && P.lora[2].A_pad && (!drop || dr.fused) && d % 256 == 0 &&
                               dkv % 256 == 0 && av_lora_batch_supported(dt, R, 3) && !av_knob(AV_KNOB_LORA_UNBATCHED);
        if (batch_bwd) {      // three launches for the three adapters' dB, dt and dA (csrc/lora_batch.hip) instead of nine
            const void* Tq[3]; long ldt3[3]; float* gBp[3]; long lgb[3]; int c0[3], nc[3];
            const void* dyp[3]; long ldy[3]; const void* BTp[3]; long lbt[3]; void* dtp[3];
            const void* dtc[3]; float* gAp[3]; long lga[3]; uint32_t sd[3];
            for (int j = 0; j < 3; ++j) {
                const avllm_lora_mod& lj = *v[j].mod;
                Tq[j] = v[j].t; dtp[j] = v[j].dt; dtc[j] = v[j].dt; ldt3[j] = v[j].ldt; sd[j] = v[j].seed;
                c0[j] = v[j].off; nc[j] = v[j].wid; lbt[j] = v[j].wid;
                dyp[j] = dqkv + (size_t)v[j].off * es; ldy[j] = qw; BTp[j] = lj.BT_pad;
                gBp[j] = lj.gB; lgb[j] = R; gAp[j] = lj.gA; lga[j] = d;
            }
            AV_TRY(av_gemm_tn_multi(dqkv, qw, qw, Tq, ldt3, gBp, lgb, c0, nc, nullptr, 3, R, M, 1.0f, 0.f, nullptr, 0, dt, st));           // dB_j = dy_j^T t_j
            AV_TRY(av_lora_rank3(dyp, ldy, nc, BTp, lbt, dtp, ldt3, nullptr, 3, M, R, m->lora_scale, 0.f, nullptr, 0, dt, st));            // dt_j = s dy_j B_j
            AV_TRY(av_gemm_tn_multi(a.xn1, d, d, dtc, ldt3, gAp, lga, nullptr, nullptr, sd, 3, R, M, 1.0f, dr.p, m->dropout_seed_dev, 1,   // dA_j = dt_j^T dropout_j(xn1)
                                    dt, st));
        } else
        for (int j = 0; j < 3; ++j)
            if (v[j].mod->A_pad) AV_TRY(lora_wgrad(m, dr, v[j], dqkv + (size_t)v[j].off * es, qw, a.xn1, w.xd, M, st));
        if (l > 0 || dx_embeds) {      // layer 0: d(inputs_embeds) only when the caller trains the connectors (frozen otherwise: SURVEY.md fact 4)
            // the second K segment takes all three adapters as one [d,192] AT image; a subset of q, k, v adds its terms one by one
            const bool seg = any && !drop && contiguous;
            g = gemm_desc(dt, w.dqkv, qw, P.wqkv_t, qw, w.dxn, d, M, d, qw);
            if (seg) { g.A2 = w.dtqkv; g.lda2 = 3 * AVLLM_LORA_PAD; g.B2 = P.lora[0].AT_pad; g.ldb2 = 3 * AVLLM_LORA_PAD; g.K2 = 3 * AVLLM_LORA_PAD; }
            AV_TRY(av_gemm(&g, st));
            if (any && !seg) AV_TRY(lora_dx_dropped(m, dr, v, 3, w.dxn, M, st));
            AV_TRY(av_rmsnorm_bwd(w.dxn, w.resid[l], P.ln1_w, a.rstd1, w.dres, l > 0 ? w.dres : dx_embeds, M, d, dt, st));      // layer 0: d resid[0]
        }
        if (after_layer) after_layer(l, user);
    }
    return AV_OK;
}

// =============================================================================================== Llama inference
namespace {
struct LlamaInferWs { void *x, *xn, *qkv, *att, *t, *gu, *hmid, *logits; float* rope_tab; float* lt; };
void carve_llama_infer(const avllm_llama* m, int B, int S, Bump& b, LlamaInferWs& w, bool all_logits) {
    const size_t es = av_dtype_size(m->dtype);
    const long M = (long)B * S;
    w.x = b.take((size_t)M * m->d * es);
    w.xn = b.take((size_t)M * m->d * es);
    w.qkv = b.take((size_t)M * llama_qw(m) * es);
    w.att = b.take((size_t)M * m->d * es);
    w.t = b.take((size_t)M * AVLLM_LORA_PAD * es);
    w.gu = b.take((size_t)M * 2 * m->ffn * es);
    w.hmid = b.take((size_t)M * m->ffn * es);
    w.logits = b.take((size_t)(all_logits ? M : B) * m->vocab * 4);
    w.rope_tab = (float*)b.take((size_t)S * (m->d / m->heads) * 4);
    w.lt = (float*)b.take((size_t)16 * 4 * AVLLM_LORA_PAD * 4);      // fused token step with adapters: rank-side products [B <= 16, 4 modules x 64] f32
}

// The code and exponent planes of layer l in an fp8 cache image (kv_fp8.hip): the codes of all layers [layers, B, Tmax, dkv] first, then the
// exponents [layers, B, Tmax, dkv/32]
struct Kv8Layer { char *kq, *ke, *vq, *ve; };
inline Kv8Layer kv8_layer(const avllm_llama* m, void* kc, void* vc, int l, int B, int Tmax) {
    const size_t dkv = (size_t)llama_dkv(m), rows = (size_t)B * Tmax, codes = (size_t)m->layers * rows * dkv;
    const size_t oq = (size_t)l * rows * dkv, oe = codes + (size_t)l * rows * (dkv >> 5);
    return {(char*)kc + oq, (char*)kc + oe, (char*)vc + oq, (char*)vc + oe};
}

// one decoder block on M = B*S rows at positions [pos0, pos0+S); K/V appended to the cache (kv_fp8: as codes + exponents; the pass's own
// attention reads its bf16 q|k|v either way)
int llama_infer_layer(const avllm_llama* m, int l, LlamaInferWs& w, int B, int S, int pos0, void* kc, void* vc, int Tmax, hipStream_t st) {
    const avllm_llama_layer& P = m->layer[l];
    const int dt = m->dtype, d = m->d, f = m->ffn, H = m->heads, hd = d / H, M = B * S;
    const int Hkv = llama_kv_heads(m), dkv = llama_dkv(m), qw = llama_qw(m);
    const size_t es = av_dtype_size(dt);
    char* kcl = (char*)kc + (size_t)l * B * Tmax * dkv * es;
    char* vcl = (char*)vc + (size_t)l * B * Tmax * dkv * es;
    AV_TRY(av_rmsnorm_fwd(w.x, P.ln1_w, w.xn, nullptr, M, d, m->eps, dt, st));
    if (!P.lora[0].A_pad && !P.lora[1].A_pad && !P.lora[2].A_pad) {      // no adapters (decode.py path): one fused q|k|v projection
        avllm_gemm_desc gq = gemm_desc(dt, w.xn, d, P.wqkv, d, w.qkv, qw, M, qw, d);
        gq.bias = P.bqkv;
        AV_TRY(av_gemm(&gq, st));
    } else
    for (int j = 0; j < 3; ++j)
        AV_TRY(lora_linear(m, w.xn, d, (const char*)P.wqkv + (size_t)llama_off(m, j) * d * es, llama_bias(m, P, j), llama_wid(m, j), P.lora[j], w.xn, 0, 0.f,
                           w.t, AVLLM_LORA_PAD, false, (char*)w.qkv + (size_t)llama_off(m, j) * es, qw, nullptr, 0, M, st));
    char* qkv = (char*)w.qkv;
    if (l == 0) AV_TRY(av_rope_table(w.rope_tab, S, hd, pos0, m->theta, st, nullptr, llama_rope_scale(m)));
    if (P.q_norm_w) AV_TRY(av_qk_norm_rope(qkv, qw, M, S, H, Hkv, hd, P.q_norm_w, P.k_norm_w, m->eps, w.rope_tab, nullptr, nullptr, nullptr, nullptr, 0, 0,
                                           nullptr, dt, st));
    else AV_TRY(av_rope_tab(qkv, qw, M, S, H + Hkv, hd, w.rope_tab, 0, dt, st));
    if (m->kv_fp8) {
        const Kv8Layer c = kv8_layer(m, kc, vc, l, B, Tmax);
        AV_TRY(av_kv8_append(qkv + (size_t)d * es, qkv + (size_t)(d + dkv) * es, qw, c.kq, c.ke, c.vq, c.ve, B, S, pos0, Tmax, dkv, st));
    } else
    AV_TRY(av_kv_append(qkv + (size_t)d * es, qkv + (size_t)(d + dkv) * es, qw, kcl, vcl, B, S, pos0, Tmax, dkv, dt, st));
    const float scale = 1.0f / sqrtf((float)hd);
    if (S == 1) {
        AV_CHECK_ARG(!m->kv_fp8, "llama: the fp8 KV cache goes with the fused token step (avllm_llama_decode_caches_fp8), not the general path");
        AV_TRY(av_attention_decode(qkv, qw, kcl, vcl, w.att, d, B, H, hd, pos0 + 1, Tmax, scale, dt, st, H / Hkv));
    } else {
        AV_CHECK_ARG(pos0 == 0, "llama prefill must start at position 0");
        AV_TRY(av_attention_fwd(qkv, qkv + (size_t)d * es, qkv + (size_t)(d + dkv) * es, w.att, nullptr, B, S, S, H, hd, qw, qw, qw,
                                d, scale, 1, dt, 0, st, Hkv));
    }
    AV_TRY(lora_linear(m, w.att, d, P.wo, P.bo, d, P.lora[3], w.att, 0, 0.f, w.t, AVLLM_LORA_PAD, false, w.x, d, w.x, d, M, st));
    AV_TRY(av_rmsnorm_fwd(w.x, P.ln2_w, w.xn, nullptr, M, d, m->eps, dt, st));
    if (!P.lora_mlp[0].A_pad && !P.lora_mlp[1].A_pad) {      // no adapter on gate or up: one fused gate|up projection
        avllm_gemm_desc g = gemm_desc(dt, w.xn, d, P.wgu, d, w.gu, 2 * f, M, 2 * f, d);
        AV_TRY(av_gemm(&g, st));
    } else
    for (int k = 0; k < 2; ++k)
        AV_TRY(lora_linear(m, w.xn, d, (const char*)P.wgu + (size_t)k * f * d * es, nullptr, f, P.lora_mlp[k], w.xn, 0, 0.f, w.t, AVLLM_LORA_PAD, false,
                           (char*)w.gu + (size_t)k * f * es, 2 * f, nullptr, 0, M, st));
    AV_TRY(av_swiglu_fwd(w.gu, w.hmid, M, f, dt, st));
    return lora_linear(m, w.hmid, f, P.wdown, nullptr, d, P.lora_mlp[2], w.hmid, 0, 0.f, w.t, AVLLM_LORA_PAD, false, w.x, d, w.x, d, M, st);
}
}  // namespace

extern "C" size_t avllm_llama_infer_workspace_bytes(const avllm_llama* m, int32_t B, int32_t S) {
    Bump b(nullptr, (size_t)-1);
    LlamaInferWs w;
    carve_llama_infer(m, B, S, b, w, true);
    return bump_size(b);
}

extern "C" int avllm_llama_prefill(const avllm_llama* m, const void* x, int32_t B, int32_t S, void* kcache, void* vcache,
                                   int32_t Tmax, float* logits_last, void* all_logits, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AV_TRY(check_llama(m));
    AV_CHECK_ARG(x && kcache && vcache && ws && B > 0 && S > 0 && S <= Tmax, "llama_prefill: bad args (S=%d Tmax=%d)", S, Tmax);
    AV_CHECK_ARG(!m->kv_fp8 || (m->dtype == AV_BF16 && (m->d / m->heads) % 64 == 0), "llama_prefill: kv_fp8 needs bf16 and a head dim of 64 or 128");
    Bump b(ws, ws_bytes);
    LlamaInferWs w;
    carve_llama_infer(m, B, S, b, w, true);
    if (!b.ok) return av_set_error(AV_ERR_WORKSPACE, "llama_prefill: workspace %zu < %zu bytes", ws_bytes, bump_size(b));
    const int dt = m->dtype, d = m->d, M = B * S;
    const size_t es = av_dtype_size(dt);
    AV_HIP(hipMemcpyAsync(w.x, x, (size_t)M * d * es, hipMemcpyDeviceToDevice, st));
    for (int l = 0; l < m->layers; ++l) AV_TRY(llama_infer_layer(m, l, w, B, S, 0, kcache, vcache, Tmax, st));
    AV_TRY(av_rmsnorm_fwd(w.x, m->norm_w, w.xn, nullptr, M, d, m->eps, dt, st));
    if (all_logits) {     // eval-mode forward(): logits for every position, in model dtype
        avllm_gemm_desc g = gemm_desc(dt, w.xn, d, m->lm_head, d, all_logits, m->vocab, M, m->vocab, d);
        AV_TRY(av_gemm(&g, st));
    }
    if (logits_last) {    // rows S-1, 2S-1, ... -> [B,vocab] f32
        avllm_gemm_desc g = gemm_desc(dt, (const char*)w.xn + (size_t)(S - 1) * d * es, (long)S * d, m->lm_head, d, logits_last, m->vocab, B, m->vocab, d);
        g.out_f32 = 1;
        AV_TRY(av_gemm(&g, st));
    }
    return AV_OK;
}

// One decoder block of a token step in 5 launches (decode.hip): bf16, B <= 16 sequences; 7 with adapters (rank <= 16: the rank-side
// products of q|k|v and of o are two more -- tiny -- launches over the A images, the B side rides in the projections' epilogues).
static bool llama_decode_lora_ok(const avllm_llama* m, const avllm_llama_layer& P, bool& any) {
    if (layer_mlp_lora(P)) { any = true; return false; }      // the epilogue form covers q, k, v, o only: merge the adapters (merge_lora) to get the fused step back
    int n = 0;
    for (int j = 0; j < 4; ++j) n += P.lora[j].A_pad != nullptr;
    any = n > 0;
    if (n == 0) return true;
    if (n != 4 || m->lora_r < 1 || m->lora_r > 16) return false;
    for (int j = 0; j < 4; ++j) if (!P.lora[j].B_pad) return false;
    // the A images of q, k, v must form one [3 x 64, d] matrix (avllm/engine.py allocates them that way): one launch makes all three products
    const size_t step = (size_t)AVLLM_LORA_PAD * m->d * 2;
    return (const char*)P.lora[1].A_pad == (const char*)P.lora[0].A_pad + step && (const char*)P.lora[2].A_pad == (const char*)P.lora[0].A_pad + 2 * step;
}
static bool llama_decode_fused_ok(const avllm_llama* m, int B) {
    const bool off = av_knob(AV_KNOB_DECODE_FUSED) == 0;
    if (off || m->dtype != AV_BF16 || B > 16) return false;
    const int hd = m->d / m->heads;
    if (!(hd == 64 || hd == 128)) return false;
    if (!av_dec_proj_supported(AV_BF16, B, m->d, llama_qw(m), 2, hd) || !av_dec_proj_supported(AV_BF16, B, m->d, m->ffn, 1, hd) ||
        !av_dec_proj_supported(AV_BF16, B, m->ffn, m->d, 0, hd) || !av_dec_proj_supported(AV_BF16, B, m->d, m->d, 0, hd)) return false;
    bool any;
    for (int l = 0; l < m->layers; ++l)
        if (!llama_decode_lora_ok(m, m->layer[l], any)) return false;      // adapters the epilogue form does not cover: the general path (lora_linear)
    return true;
}

// The weights one projection of the token step streams, in the model's form: bf16 rows of K, or with decode_fp8 / decode_fp4 the e4m3 / MXFP4
// codes (two per byte: the row stride halves) with their exponents (decode.hip)
static void dec_weights(const avllm_llama* m, avllm_dec_proj_desc& p, int K, const void* W, const void* W8, const void* E8, const void* W4, const void* E4) {
    p.W = W; p.ldw = K;
    if (m->decode_fp8) { p.W8 = W8; p.E8 = E8; }
    if (m->decode_fp4) { p.W4 = W4; p.E8 = E4; p.ldw = K / 2; }
}

// The prefix of a shared-prefix token step (avllm_llama_decode_step_shared): the step's B rows are `group` rows per item of the rows-row cache
// kp / vp [layers, rows, S, dkv] the prefill wrote; kc / vc of the layer function are then the suffix caches, Tmax their N, pos the suffix row.
struct SharedPrefix { const void *kp, *vp; int rows, S, group; void* ws; size_t ws_bytes; };

static int llama_decode_layer_fused(const avllm_llama* m, int l, LlamaInferWs& w, int B, int pos, const int* pos_dev, void* kc, void* vc, int Tmax,
                                    hipStream_t st, const SharedPrefix* sp = nullptr) {
    const avllm_llama_layer& P = m->layer[l];
    const int d = m->d, f = m->ffn, H = m->heads, hd = d / H, Hkv = llama_kv_heads(m), dkv = llama_dkv(m), qw = llama_qw(m);
    char* kcl = (char*)kc + (size_t)l * B * Tmax * dkv * 2;
    char* vcl = (char*)vc + (size_t)l * B * Tmax * dkv * 2;
    bool lora = false;
    llama_decode_lora_ok(m, P, lora);
    constexpr int LT = 4 * AVLLM_LORA_PAD;
    avllm_dec_proj_desc p = {};
    if (lora) {      // lora_A(rmsnorm(x)) of q, k, v in one launch over the stacked A images [3 x 64, d] -> lt[:, 0:192]
        p.A = w.x; p.lda = d; p.W = P.lora[0].A_pad; p.ldw = d; p.norm_w = P.ln1_w; p.eps = m->eps; p.M = B; p.K = d; p.N = 3 * AVLLM_LORA_PAD; p.mode = 0;
        p.C = w.lt; p.ldc = LT; p.out_f32 = 1;
        AV_TRY(av_dec_proj(&p, st));
        p = {};
    }
    dec_weights(m, p, d, P.wqkv, P.wqkv8, P.eqkv8, P.wqkv4, P.eqkv4);
    p.A = w.x; p.lda = d; p.norm_w = P.ln1_w; p.eps = m->eps; p.M = B; p.K = d; p.N = qw; p.mode = 2;
    p.C = w.qkv; p.ldc = qw; p.dq = d; p.dkv = dkv; p.hd = hd; p.rope = w.rope_tab; p.kc = kcl; p.vc = vcl; p.Tmax = Tmax; p.pos = pos; p.pos_dev = pos_dev;
    p.bias = P.bqkv;
    if (lora) {
        p.lora_t = w.lt; p.ld_lora_t = LT; p.lora_r = m->lora_r; p.lora_scale = m->lora_scale;
        for (int j = 0; j < 3; ++j) p.lora_b[j] = P.lora[j].B_pad;
    }
    // head norms: a head's columns belong to hd / 16 workgroups of the projection, so q|k|v leave it raw and one launch normalises, rotates
    // and writes the cache row (6 launches per layer, 8 with adapters)
    // fp8 cache: an MX block is 32 columns of a row, two workgroups of the projection, so q|k|v leave it raw here too and one launch rotates,
    // quantises and writes the row (one launch more per layer; with head norms their launch rotates in place and the append follows: two more)
    p.raw_qkv = P.q_norm_w != nullptr || m->kv_fp8;
    AV_TRY(av_dec_proj(&p, st));
    if (m->kv_fp8) {
        const Kv8Layer c = kv8_layer(m, kc, vc, l, B, Tmax);
        if (P.q_norm_w) AV_TRY(av_qk_norm_rope(w.qkv, qw, B, 1, H, Hkv, hd, P.q_norm_w, P.k_norm_w, m->eps, w.rope_tab, nullptr, nullptr, nullptr, nullptr, 0, 0,
                                               nullptr, AV_BF16, st));
        AV_TRY(av_kv8_rope_append(w.qkv, qw, B, H, Hkv, hd, w.rope_tab, P.q_norm_w == nullptr, c.kq, c.ke, c.vq, c.ve, Tmax, pos, pos_dev, st));
        if (sp) {
            const Kv8Layer c0 = kv8_layer(m, const_cast<void*>(sp->kp), const_cast<void*>(sp->vp), l, sp->rows, sp->S);
            AV_TRY(av_attention_decode_shared_kv8(w.qkv, qw, c0.kq, c0.ke, c0.vq, c0.ve, sp->S, sp->S, c.kq, c.ke, c.vq, c.ve, pos + 1, pos_dev, Tmax, w.att, d, B,
                                                  sp->group, H, hd, 1.0f / sqrtf((float)hd), H / Hkv, sp->ws, sp->ws_bytes, st));
        } else
        AV_TRY(av_attention_decode_kv8(w.qkv, qw, c.kq, c.ke, c.vq, c.ve, w.att, d, B, H, hd, pos + 1, pos_dev, Tmax, 1.0f / sqrtf((float)hd), H / Hkv, st));
    } else {
        if (P.q_norm_w) AV_TRY(av_qk_norm_rope(w.qkv, qw, B, 1, H, Hkv, hd, P.q_norm_w, P.k_norm_w, m->eps, w.rope_tab, nullptr, nullptr, kcl, vcl, Tmax, pos,
                                               pos_dev, AV_BF16, st));
        if (sp) {
            const size_t off = (size_t)l * sp->rows * sp->S * dkv * 2;
            AV_TRY(av_attention_decode_shared(w.qkv, qw, (const char*)sp->kp + off, (const char*)sp->vp + off, sp->S, sp->S, kcl, vcl, pos + 1, pos_dev, Tmax, w.att,
                                              d, B, sp->group, H, hd, 1.0f / sqrtf((float)hd), H / Hkv, sp->ws, sp->ws_bytes, st));
        } else
        AV_TRY(av_attention_decode1(w.qkv, qw, kcl, vcl, w.att, d, B, H, hd, pos + 1, pos_dev, Tmax, 1.0f / sqrtf((float)hd), AV_BF16, st, H / Hkv));
    }
    p = {};
    if (lora) {      // lora_A(attention output) -> lt[:, 192:192+16]: only the rank's own 16 rows of the padded image are streamed
        p.A = w.att; p.lda = d; p.W = P.lora[3].A_pad; p.ldw = d; p.M = B; p.K = d; p.N = 16; p.mode = 0; p.C = w.lt + 3 * AVLLM_LORA_PAD; p.ldc = LT; p.out_f32 = 1;
        AV_TRY(av_dec_proj(&p, st));
        p = {};
    }
    dec_weights(m, p, d, P.wo, P.wo8, P.eo8, P.wo4, P.eo4);
    p.A = w.att; p.lda = d; p.M = B; p.K = d; p.N = d; p.mode = 0; p.C = w.x; p.ldc = d; p.R = w.x; p.ldr = d; p.bias = P.bo;
    if (lora) { p.lora_t = w.lt + 3 * AVLLM_LORA_PAD; p.ld_lora_t = LT; p.lora_r = m->lora_r; p.lora_scale = m->lora_scale; p.lora_b[0] = P.lora[3].B_pad; }
    AV_TRY(av_dec_proj(&p, st));
    p = {};
    dec_weights(m, p, d, P.wgu, P.wgu8, P.egu8, P.wgu4, P.egu4);
    p.A = w.x; p.lda = d; p.norm_w = P.ln2_w; p.eps = m->eps; p.M = B; p.K = d; p.N = f; p.mode = 1; p.C = w.hmid; p.ldc = f;
    AV_TRY(av_dec_proj(&p, st));
    p = {};
    dec_weights(m, p, f, P.wdown, P.wdown8, P.edown8, P.wdown4, P.edown4);
    p.A = w.hmid; p.lda = f; p.M = B; p.K = f; p.N = d; p.mode = 0; p.C = w.x; p.ldc = d; p.R = w.x; p.ldr = d;
    return av_dec_proj(&p, st);
}

// final norm + lm_head of a token step -> logits [B, vocab] f32.  fold: the norm rides in the lm_head stream (fused step, where dec_proj takes the vocab)
static int llama_decode_head(const avllm_llama* m, LlamaInferWs& w, int B, float* logits, bool fold, hipStream_t st) {
    const int dt = m->dtype, d = m->d;
    if (fold && av_dec_proj_supported(AV_BF16, B, d, m->vocab, 0, 0)) {
        avllm_dec_proj_desc p = {};
        p.A = w.x; p.lda = d; p.W = m->lm_head; p.ldw = d; p.norm_w = m->norm_w; p.eps = m->eps; p.M = B; p.K = d; p.N = m->vocab; p.mode = 0;
        p.C = logits; p.ldc = m->vocab; p.out_f32 = 1;
        if (m->decode_fp8 || m->decode_fp4) { p.W8 = m->lm_head8; p.E8 = m->elm_head8; }      // decode_fp4: lm_head stays e4m3
        return av_dec_proj(&p, st);
    }
    AV_TRY(av_rmsnorm_fwd(w.x, m->norm_w, w.xn, nullptr, B, d, m->eps, dt, st));
    avllm_gemm_desc g = gemm_desc(dt, w.xn, d, m->lm_head, d, logits, m->vocab, B, m->vocab, d);
    g.out_f32 = 1;
    return av_gemm(&g, st);
}

extern "C" int avllm_llama_decode_step_at(const avllm_llama* m, const int64_t* ids, int32_t B, int32_t pos, const int32_t* pos_dev, void* kcache,
                                          void* vcache, int32_t Tmax, float* logits, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AV_TRY(check_llama(m));
    AV_CHECK_ARG(ids && kcache && vcache && logits && ws && B > 0 && pos >= 0 && (pos_dev || pos < Tmax), "llama_decode_step: bad args (pos=%d Tmax=%d)", pos, Tmax);
    Bump b(ws, ws_bytes);
    LlamaInferWs w;
    carve_llama_infer(m, B, 1, b, w, true);
    if (!b.ok) return av_set_error(AV_ERR_WORKSPACE, "llama_decode_step: workspace %zu < %zu bytes", ws_bytes, bump_size(b));
    const int dt = m->dtype, d = m->d;
    AV_TRY(av_embedding(m->embed, ids, w.x, B, d, dt, st));
    AV_CHECK_ARG(!m->kv_fp8 || llama_decode_fused_ok(m, B),
                 "llama_decode_step: kv_fp8 needs the fused token step (bf16, B <= 16 (B=%d), head dim 64 or 128): see avllm_llama_decode_caches_fp8", B);
    const bool fused = llama_decode_fused_ok(m, B);
    if (fused) {
        AV_TRY(av_rope_table(w.rope_tab, 1, d / m->heads, pos, m->theta, st, pos_dev, llama_rope_scale(m)));
        for (int l = 0; l < m->layers; ++l) AV_TRY(llama_decode_layer_fused(m, l, w, B, pos, pos_dev, kcache, vcache, Tmax, st));
    } else {
        AV_CHECK_ARG(!pos_dev, "llama_decode_step: a device-side position needs the fused bf16 token step (B <= 16, adapters of rank <= 16 or none)");
        for (int l = 0; l < m->layers; ++l) AV_TRY(llama_infer_layer(m, l, w, B, 1, pos, kcache, vcache, Tmax, st));
    }
    return llama_decode_head(m, w, B, logits, fused, st);
}

// The token step of R = B group rows whose items' prefixes [0, S) are stored once (k_prefix / v_prefix: the R / group-row cache of S positions the
// prefill wrote).  Fused path only.  Only the attention launch differs from avllm_llama_decode_step_at: the RoPE table is that of position
// S + pos, the cache row written is `pos` of the suffix caches [layers, R, N, dkv] (both + *pos_dev), by the same writers.
extern "C" size_t avllm_llama_decode_shared_workspace_bytes(const avllm_llama* m, int32_t R) {
    Bump b(nullptr, (size_t)-1);
    LlamaInferWs w;
    carve_llama_infer(m, R, 1, b, w, true);
    b.take(av_attention_decode_shared_ws(R, m->heads, m->d / m->heads));
    return bump_size(b);
}

extern "C" int avllm_llama_decode_step_shared(const avllm_llama* m, const int64_t* ids, int32_t R, int32_t group, int32_t pos, const int32_t* pos_dev,
                                              const void* k_prefix, const void* v_prefix, int32_t S, void* k_suffix, void* v_suffix, int32_t N, float* logits,
                                              void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AV_TRY(check_llama(m));
    AV_CHECK_ARG(ids && logits && ws, "llama_decode_step_shared: ids, logits or ws is null");
    AV_CHECK_ARG(k_prefix && v_prefix && S > 0, "llama_decode_step_shared: k_prefix / v_prefix null or S=%d not positive", S);
    AV_CHECK_ARG(k_suffix && v_suffix && N > 0, "llama_decode_step_shared: k_suffix / v_suffix null or N=%d not positive", N);
    AV_CHECK_ARG(R > 0 && group > 0 && R % group == 0, "llama_decode_step_shared: R=%d rows must be whole groups of group=%d", R, group);
    AV_CHECK_ARG(pos >= 0 && (pos_dev || pos < N), "llama_decode_step_shared: pos=%d outside the suffix cache (N=%d)", pos, N);
    AV_CHECK_ARG(llama_decode_fused_ok(m, R),
                 "llama_decode_step_shared: needs the fused token step (bf16, R <= 16 (R=%d), head dim 64 or 128): see avllm_llama_decode_shares_prefix", R);
    Bump b(ws, ws_bytes);
    LlamaInferWs w;
    carve_llama_infer(m, R, 1, b, w, true);
    SharedPrefix sp = {k_prefix, v_prefix, R / group, S, group, nullptr, av_attention_decode_shared_ws(R, m->heads, m->d / m->heads)};
    sp.ws = b.take(sp.ws_bytes);
    if (!b.ok) return av_set_error(AV_ERR_WORKSPACE, "llama_decode_step_shared: workspace %zu < %zu bytes", ws_bytes, bump_size(b));
    const int d = m->d;
    AV_TRY(av_embedding(m->embed, ids, w.x, R, d, m->dtype, st));
    AV_TRY(av_rope_table(w.rope_tab, 1, d / m->heads, S + pos, m->theta, st, pos_dev, llama_rope_scale(m)));
    for (int l = 0; l < m->layers; ++l) AV_TRY(llama_decode_layer_fused(m, l, w, R, pos, pos_dev, k_suffix, v_suffix, N, st, &sp));
    return llama_decode_head(m, w, R, logits, true, st);
}

// sharing goes with the fused step, as the weight and cache forms do
extern "C" int avllm_llama_decode_shares_prefix(const avllm_llama* m, int32_t R) { return m && check_llama(m) == AV_OK && llama_decode_fused_ok(m, R) ? 1 : 0; }

extern "C" int avllm_llama_decode_is_fused(const avllm_llama* m, int32_t B) { return m && check_llama(m) == AV_OK && llama_decode_fused_ok(m, B) ? 1 : 0; }
// decode_fp8 is honoured on the fused path only (check_llama guarantees vocab % 16 == 0, so lm_head is folded there too); B > 16 and a
// disabled fused path read the bf16 matrices
extern "C" int avllm_llama_decode_streams_fp8(const avllm_llama* m, int32_t B) {
    return m && check_llama(m) == AV_OK && m->decode_fp8 && llama_decode_fused_ok(m, B) ? 1 : 0;
}
extern "C" int avllm_llama_decode_streams_fp4(const avllm_llama* m, int32_t B) {
    return m && check_llama(m) == AV_OK && m->decode_fp4 && llama_decode_fused_ok(m, B) ? 1 : 0;
}

// the fp8 cache goes with the fused step, as the weight forms do
extern "C" int avllm_llama_decode_caches_fp8(const avllm_llama* m, int32_t B) {
    return m && check_llama(m) == AV_OK && m->kv_fp8 && llama_decode_fused_ok(m, B) ? 1 : 0;
}
extern "C" size_t avllm_llama_kv_cache_bytes(const avllm_llama* m, int32_t B, int32_t Tmax) {
    if (!m || check_llama(m) != AV_OK || B <= 0 || Tmax <= 0) return 0;
    const size_t n = (size_t)m->layers * B * Tmax * llama_dkv(m);
    return m->kv_fp8 ? n + n / 32 : n * av_dtype_size(m->dtype);
}

extern "C" int avllm_llama_decode_step(const avllm_llama* m, const int64_t* ids, int32_t B, int32_t pos, void* kcache,
                                       void* vcache, int32_t Tmax, float* logits, void* ws, size_t ws_bytes, void* stream) {
    return avllm_llama_decode_step_at(m, ids, B, pos, nullptr, kcache, vcache, Tmax, logits, ws, ws_bytes, stream);
}
