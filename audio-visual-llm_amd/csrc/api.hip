// extern "C" surface of libavllm.so (include/avllm.h): error string + thin wrappers that turn the void*
// stream into a hipStream_t.  No torch types, no allocation.
#include "common.h"
#include "avllm_internal.h"
#include <stdarg.h>

static thread_local char g_err[512] = "";

int av_set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ---- experiment knobs (common.h AvKnob)
#include <mutex>
#include <string.h>
static const struct { const char* name; int dflt; } g_knob_def[AV_KNOB_COUNT] = {
    {"DECODE_FUSED", 1}, {"DEC_AL", 0}, {"LORA_UNBATCHED", 0}, {"F8_UNFUSED_QUANT", 0}, {"F8_FAST", 1}, {"ATTN_SHORT", 1},
    {"NARROW_EPILOGUE", 0}, {"TN_CHUNK", 0}, {"GEMM_DBG", 0}, {"GEMM_GW", 0}, {"GEMM_VARIANT", 0}, {"SHARED_SPLIT", 0}};
static int g_knob[AV_KNOB_COUNT];
static std::once_flag g_knob_once;
static void knob_init() {
    for (int i = 0; i < AV_KNOB_COUNT; ++i) {
        char env[64];
        snprintf(env, sizeof(env), "AVLLM_%s", g_knob_def[i].name);
        const char* e = getenv(env);
        g_knob[i] = e ? atoi(e) : g_knob_def[i].dflt;
    }
}
int av_knob(int id) {
    std::call_once(g_knob_once, knob_init);
    return g_knob[id];
}
static int* knob_slot(const char* name) {
    std::call_once(g_knob_once, knob_init);
    for (int i = 0; name && i < AV_KNOB_COUNT; ++i)
        if (!strcmp(name, g_knob_def[i].name)) return &g_knob[i];
    return nullptr;
}

int av_device(int* ncu) {
    static int g_ncu[AV_MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const int slot = dev & (AV_MAX_DEVICES - 1);
    if (!g_ncu[slot] && hipDeviceGetAttribute(&g_ncu[slot], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) g_ncu[slot] = 256;
    *ncu = g_ncu[slot];
    return slot;
}

#define ST ((hipStream_t)stream)
extern "C" {
int avllm_set_knob(const char* name, int32_t value) {
    int* k = knob_slot(name);
    AV_CHECK_ARG(k, "set_knob: unknown knob '%s'", name ? name : "(null)");
    *k = value;
    return AV_OK;
}
int avllm_get_knob(const char* name, int32_t* value) {
    const int* k = knob_slot(name);
    AV_CHECK_ARG(k && value, "get_knob: unknown knob '%s'", name ? name : "(null)");
    *value = *k;
    return AV_OK;
}
int avllm_set_gemm_variant(int v) { return avllm_set_knob("GEMM_VARIANT", v); }
const char* avllm_last_error(void) { return g_err; }
int avllm_version(void) { return 100; }

int avllm_gemm(const avllm_gemm_desc* d, void* stream) { return av_gemm(d, ST); }
int avllm_gemm_plan(const avllm_gemm_desc* d, int32_t* kernel) { AV_CHECK_ARG(kernel, "gemm_plan: null kernel"); return av_gemm_plan(d, kernel); }
int avllm_gemm_tn(const void* P, int64_t ldp, int32_t I, const void* Q, int64_t ldq, int32_t J, int32_t M, float* out,
                  int64_t ldo, float alpha, int32_t dtype, void* stream) { return av_gemm_tn(P, ldp, I, Q, ldq, J, M, out, ldo, alpha, dtype, ST); }
int avllm_gemm_tn_drop(const void* P, int64_t ldp, int32_t I, const void* Q, int64_t ldq, int32_t J, int32_t M, float* out,
                       int64_t ldo, float alpha, uint32_t seed, float p, int32_t dtype, void* stream) { return av_gemm_tn(P, ldp, I, Q, ldq, J, M, out, ldo, alpha, dtype, ST, seed, p); }
int avllm_layernorm(const void* x, const void* w, const void* b, void* y, int64_t rows, int32_t d, float eps, int32_t dtype,
                    void* stream) { return av_layernorm(x, w, b, y, rows, d, eps, dtype, ST); }
int avllm_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int64_t rows, int32_t d, float eps, int32_t dtype,
                      void* stream) { return av_rmsnorm_fwd(x, w, y, rstd, rows, d, eps, dtype, ST); }
int avllm_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, const void* dres_in, void* dx_out,
                      int64_t rows, int32_t d, int32_t dtype, void* stream) { return av_rmsnorm_bwd(dy, x, w, rstd, dres_in, dx_out, rows, d, dtype, ST); }
int avllm_rope(void* x, int64_t ld, int64_t rows, int32_t T, int32_t heads, int32_t hd, int32_t pos0, float theta,
               int32_t inverse, int32_t dtype, void* stream) { return av_rope(x, ld, rows, T, heads, hd, pos0, theta, inverse, dtype, ST); }
int avllm_rope_table(float* tab, int32_t T, int32_t hd, int32_t pos0, float theta, const int32_t* pos_dev, float factor,
                     float low_freq_factor, float high_freq_factor, int32_t orig_ctx, void* stream) {
    AvRopeScale sc;
    sc.factor = factor; sc.low_freq_factor = low_freq_factor; sc.high_freq_factor = high_freq_factor; sc.orig_ctx = orig_ctx;
    AV_CHECK_ARG(orig_ctx <= 0 || (factor > 0.f && low_freq_factor > 0.f && high_freq_factor > low_freq_factor), "rope_table: bad llama3 scaling");
    return av_rope_table(tab, T, hd, pos0, theta, ST, pos_dev, sc);
}
int avllm_rope_tab(void* x, int64_t ld, int64_t rows, int32_t T, int32_t heads, int32_t hd, const float* tab, int32_t inverse,
                   int32_t dtype, void* stream) { return av_rope_tab(x, ld, rows, T, heads, hd, tab, inverse, dtype, ST); }
int avllm_kv_append(const void* k, const void* v, int64_t ld, void* kc, void* vc, int32_t B, int32_t T, int32_t pos0, int32_t Tmax,
                    int32_t d, int32_t dtype, void* stream) { return av_kv_append(k, v, ld, kc, vc, B, T, pos0, Tmax, d, dtype, ST); }
int avllm_swiglu_fwd(const void* gu, void* h, int64_t M, int32_t F, int32_t dtype, void* stream) { return av_swiglu_fwd(gu, h, M, F, dtype, ST); }
int avllm_swiglu_bwd(const void* dh, const void* gu, void* dgu, int64_t M, int32_t F, int32_t dtype, void* stream) { return av_swiglu_bwd(dh, gu, dgu, M, F, dtype, ST); }
int avllm_swiglu_bwd_h(const void* dh, const void* gu, void* dgu, void* h, int64_t M, int32_t F, int32_t dtype, void* stream) { return av_swiglu_bwd_h(dh, gu, dgu, h, M, F, dtype, ST); }
int avllm_attention_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int32_t B, int32_t Tq, int32_t Tk,
                        int32_t H, int32_t hd, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, int32_t causal,
                        int32_t dtype, int32_t impl, int32_t kv_heads, void* stream) {
    return av_attention_fwd(q, k, v, o, lse, B, Tq, Tk, H, hd, ldq, ldk, ldv, ldo, scale, causal, dtype, impl, ST, kv_heads);
}
int avllm_attention_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, void* dq,
                        void* dk, void* dv, float* delta_ws, int32_t B, int32_t T, int32_t H, int32_t hd, int64_t ldq, int64_t ldk,
                        int64_t ldv, int64_t ldo, int64_t lddq, int64_t lddk, int64_t lddv, float scale, int32_t causal,
                        int32_t dtype, int32_t impl, int32_t kv_heads, void* stream) {
    return av_attention_bwd(q, k, v, o, dout, lse, dq, dk, dv, delta_ws, B, T, H, hd, ldq, ldk, ldv, ldo, lddq, lddk, lddv, scale, causal, dtype, impl, ST, kv_heads);
}
int avllm_attention_bwd_rope(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, void* dq,
                             void* dk, void* dv, float* delta_ws, int32_t B, int32_t T, int32_t H, int32_t hd, int64_t ldq, int64_t ldk,
                             int64_t ldv, int64_t ldo, int64_t lddq, int64_t lddk, int64_t lddv, float scale, int32_t causal,
                             int32_t dtype, int32_t impl, int32_t kv_heads, const float* rope_tab, void* stream) {
    return av_attention_bwd(q, k, v, o, dout, lse, dq, dk, dv, delta_ws, B, T, H, hd, ldq, ldk, ldv, ldo, lddq, lddk, lddv, scale, causal, dtype, impl, ST, kv_heads, rope_tab);
}
int avllm_ce_fwd(const void* logits, int64_t ld, const int64_t* labels, int32_t B, int32_t T, int32_t V, float* row_lse,
                 float* loss_sum, float* count, int32_t dtype, void* stream) { return av_ce_fwd(logits, ld, labels, B, T, V, row_lse, loss_sum, count, dtype, ST); }
int avllm_ce_smooth_fwd(const void* logits, int64_t ld, const int64_t* labels, int32_t B, int32_t T, int32_t V, float label_smoothing, float z_loss,
                        float* row_lse, float* loss_sum, float* count, float* terms, int32_t dtype, void* stream) {
    return av_ce_smooth_fwd(logits, ld, labels, B, T, V, label_smoothing, z_loss, row_lse, loss_sum, count, terms, dtype, ST);
}
int avllm_ce_smooth_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* row_lse, const float* count, float grad_scale,
                        float label_smoothing, float z_loss, void* dlogits, int32_t B, int32_t T, int32_t V, int32_t dtype, void* stream) {
    return av_ce_smooth_bwd(logits, ld, labels, row_lse, count, grad_scale, label_smoothing, z_loss, dlogits, B, T, V, dtype, ST);
}
int avllm_ce_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* row_lse, const float* count, float grad_scale,
                 void* dlogits, int32_t B, int32_t T, int32_t V, int32_t dtype, void* stream) { return av_ce_bwd(logits, ld, labels, row_lse, count, grad_scale, dlogits, B, T, V, dtype, ST); }
int avllm_argmax_rows(const void* logits, int64_t ld, int64_t rows, int32_t V, int64_t* out, int32_t dtype, void* stream) { return av_argmax_rows(logits, ld, rows, V, out, dtype, ST); }
int avllm_sample_rows(const void* logits, int64_t ld, int64_t rows, int32_t V, float temperature, int32_t top_k, float top_p, uint32_t seed,
                      const uint32_t* row_seeds, int32_t step, const int32_t* step_dev, uint8_t* unfinished, int64_t eos, int64_t pad,
                      int64_t* out, int32_t dtype, void* stream) {
    return av_sample_rows(logits, ld, rows, V, temperature, top_k, top_p, seed, row_seeds, step, step_dev, unfinished, eos, pad, out, nullptr, dtype, ST);
}
int avllm_sample_rows_scored(const void* logits, int64_t ld, int64_t rows, int32_t V, float temperature, int32_t top_k, float top_p, uint32_t seed,
                             const uint32_t* row_seeds, int32_t step, const int32_t* step_dev, uint8_t* unfinished, int64_t eos, int64_t pad,
                             int64_t* out, float* out_logprob, int32_t dtype, void* stream) {
    return av_sample_rows(logits, ld, rows, V, temperature, top_k, top_p, seed, row_seeds, step, step_dev, unfinished, eos, pad, out, out_logprob, dtype,
                          ST);
}
int avllm_row_scores(const void* logits, int64_t ld, int64_t rows, int32_t V, const int64_t* tokens, float temperature, float* out_logprob,
                     float* out_entropy, int32_t dtype, void* stream) {
    return av_row_scores(logits, ld, rows, V, tokens, temperature, out_logprob, out_entropy, 0, dtype, ST);
}
int avllm_row_scores_logprobs(const void* logprobs, int64_t ld, int64_t rows, int32_t V, const int64_t* tokens, float* out_logprob,
                              float* out_entropy, int32_t dtype, void* stream) {
    return av_row_scores(logprobs, ld, rows, V, tokens, 1.0f, out_logprob, out_entropy, 1, dtype, ST);
}
size_t avllm_beam_topk_workspace_bytes(int64_t rows, int32_t V, int32_t k) { return av_beam_topk_workspace_bytes(rows, V, k); }
int avllm_beam_topk(const float* logits, int64_t ld, int32_t B, int32_t num_beams, int32_t V, const float* beam_scores, int32_t k,
                    float* out_scores, int32_t* out_beams, int64_t* out_tokens, void* ws, size_t ws_bytes, void* stream) {
    return av_beam_topk(logits, ld, B, num_beams, V, beam_scores, k, out_scores, out_beams, out_tokens, ws, ws_bytes, 0, ST);
}
int avllm_beam_topk_logprobs(const float* logprobs, int64_t ld, int32_t B, int32_t num_beams, int32_t V, const float* beam_scores, int32_t k,
                             float* out_scores, int32_t* out_beams, int64_t* out_tokens, void* ws, size_t ws_bytes, void* stream) {
    return av_beam_topk(logprobs, ld, B, num_beams, V, beam_scores, k, out_scores, out_beams, out_tokens, ws, ws_bytes, 1, ST);
}
int avllm_logits_process(void* scores, int64_t ld, int64_t rows, int32_t V, int64_t* history, int64_t ldh, const int64_t* append, int32_t cur,
                         const int32_t* cur_dev, float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_new_tokens, int64_t eos,
                         int32_t log_softmax, int32_t dtype, void* stream) {
    avllm_logits_proc_desc d = {};                 // no tables: the descriptor entry below with every n_* zero
    d.scores = scores; d.ld = ld; d.rows = rows; d.V = V; d.dtype = dtype;
    d.history = history; d.ldh = ldh; d.append = append; d.cur = cur; d.cur_dev = cur_dev;
    d.repetition_penalty = repetition_penalty; d.no_repeat_ngram_size = no_repeat_ngram_size; d.min_new_tokens = min_new_tokens;
    d.eos = eos; d.log_softmax = log_softmax;
    return av_logits_process(&d, ST);
}
int avllm_logits_process_ex(const avllm_logits_proc_desc* d, void* stream) { return av_logits_process(d, ST); }
int avllm_kv_gather_rows(const void* k_src, const void* v_src, int32_t src_rows, int64_t src_T, void* k_dst, void* v_dst, int32_t dst_rows,
                         int64_t dst_T, int32_t layers, int32_t dkv, const int32_t* parent, int32_t t0, int32_t t1, int32_t dtype, void* stream) {
    return av_kv_gather_rows(k_src, v_src, src_rows, src_T, k_dst, v_dst, dst_rows, dst_T, layers, dkv, parent, t0, t1, dtype, ST);
}
int avllm_embedding(const void* table, const int64_t* ids, void* out, int64_t n, int32_t d, int32_t dtype, void* stream) { return av_embedding(table, ids, out, n, d, dtype, ST); }
int avllm_cast(const void* src, int32_t sdt, void* dst, int32_t ddt, int64_t n, void* stream) { return av_cast(src, sdt, dst, ddt, n, ST); }
int avllm_dropout(const void* x, void* y, int64_t rows, int32_t d, uint32_t seed, float p, int32_t dtype, void* stream) { return av_dropout(x, y, rows, d, seed, p, dtype, ST); }
int avllm_whisper_im2col1(const float* mel, void* cols, int32_t B, int32_t n_mels, int32_t T, int32_t Kpad, int32_t dtype, void* stream) { return av_whisper_im2col1(mel, cols, B, n_mels, T, Kpad, dtype, ST); }
int avllm_whisper_im2col2(const void* h, void* cols, int32_t B, int32_t T, int32_t d, int32_t dtype, void* stream) { return av_whisper_im2col2(h, cols, B, T, d, dtype, ST); }
int avllm_clip_patchify(const float* frames, void* cols, int32_t N, int32_t S, int32_t p, int32_t Kpad, int32_t dtype, void* stream) { return av_clip_patchify(frames, cols, N, S, p, Kpad, dtype, ST); }
int avllm_clip_cls_rows(const void* ce, const void* pos, void* x, int32_t N, int32_t tokens, int32_t d, int32_t dtype, void* stream) { return av_clip_cls_rows(ce, pos, x, N, tokens, d, dtype, ST); }
int avllm_fuse_pool(const void* a, int32_t Ta, const void* v, int32_t Tv, const void* pe, int32_t P, void* out, int32_t B, int32_t L,
                    int32_t S_out, int32_t D, float fs, int32_t dtype, void* stream) { return av_fuse_pool(a, Ta, v, Tv, pe, P, out, B, L, S_out, D, fs, dtype, ST); }
int avllm_fuse_pool_bwd(const void* dx, void* da, int32_t Ta, void* dv, int32_t Tv, int32_t P, int32_t B, int32_t L, int32_t S_out, int32_t D,
                        float fs, int32_t dtype, void* stream) { return av_fuse_pool_bwd(dx, da, Ta, dv, Tv, P, B, L, S_out, D, fs, dtype, ST); }
int avllm_fuse_pool_rows(const void* a, int32_t Ta, const void* v, int32_t Tv, const void* pe, int32_t P, const int32_t* mode, void* out, int32_t B,
                         int32_t L, int32_t S_out, int32_t D, float fs, int32_t dtype, void* stream) {
    return av_fuse_pool_rows(a, Ta, v, Tv, pe, P, mode, out, B, L, S_out, D, fs, dtype, ST);
}
int avllm_fuse_pool_rows_bwd(const void* dx, void* da, int32_t Ta, void* dv, int32_t Tv, int32_t P, const int32_t* mode, int32_t B, int32_t L,
                             int32_t S_out, int32_t D, float fs, int32_t dtype, void* stream) {
    return av_fuse_pool_rows_bwd(dx, da, Ta, dv, Tv, P, mode, B, L, S_out, D, fs, dtype, ST);
}
int avllm_modality_draw(const int32_t* mode_in, int32_t* mode_out, int32_t B, float p_drop_audio, float p_drop_video, uint32_t seed,
                        const uint32_t* seed_dev, void* stream) { return av_modality_draw(mode_in, mode_out, B, p_drop_audio, p_drop_video, seed, seed_dev, ST); }
int avllm_gemm_wgrad(const void* dY, int64_t ldy, const void* X, int64_t ldx, int32_t M, int32_t N, int32_t K, float* dW, int64_t ldw, float* db,
                     float alpha, int32_t dtype, void* stream) { return av_gemm_wgrad(dY, ldy, X, ldx, M, N, K, dW, ldw, db, alpha, dtype, ST); }
int avllm_grad_sumsq_det_multi(const float* const* g, const int64_t* n, int32_t nbuf, float* partials, int32_t nparts, float* sumsq, void* stream) {
    return av_grad_sumsq_det_multi(g, n, nbuf, partials, nparts, sumsq, ST);
}
int avllm_adamw_step_multi(const avllm_adamw_seg* segs, int32_t nseg, float lr, float b1, float b2, float eps, int32_t step, const float* sumsq,
                           float max_norm, float prescale, const float* guard, float* skipped, const avllm_step_state* state, void* stream) {
    return av_adamw_step_multi(segs, nseg, lr, b1, b2, eps, step, sumsq, max_norm, prescale, guard, skipped, state, ST);
}
int avllm_grad_sumsq(const float* g, int64_t n, float* sumsq, void* stream) { return av_grad_sumsq(g, n, sumsq, ST); }
int avllm_grad_sumsq_det(const float* g, int64_t n, float* partials, int32_t nparts, float* sumsq, void* stream) { return av_grad_sumsq_det(g, n, partials, nparts, sumsq, ST); }
int avllm_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                     int32_t step, const float* sumsq, float max_norm, float prescale, const float* guard, float* skipped,
                     const avllm_step_state* state, void* stream) {
    return av_adamw_step(p, g, m, v, n, lr, b1, b2, eps, wd, step, sumsq, max_norm, prescale, guard, skipped, state, ST);
}
int avllm_act_residual(const void* x, const void* r, void* y, int64_t n, int32_t act, int32_t dtype, void* stream) { return av_act_residual(x, r, y, n, act, dtype, ST); }
int avllm_step_advance(avllm_step_state* state, const avllm_schedule* sched, void* stream) { return av_step_advance(state, sched, ST); }
int avllm_gemm_wgrad_acc(const void* dY, int64_t ldy, const void* X, int64_t ldx, int32_t M, int32_t N, int32_t K, float* dW, int64_t ldw, float* db,
                         float alpha, int32_t dtype, void* stream) { return av_gemm_wgrad_acc(dY, ldy, X, ldx, M, N, K, dW, ldw, db, alpha, dtype, ST); }
int avllm_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                         int32_t step, const float* sumsq, float max_norm, const float* grad_div_dev, const float* guard, float* skipped,
                         const avllm_step_state* state, void* stream) {
    return av_adamw_step_dev(p, g, m, v, n, lr, b1, b2, eps, wd, step, sumsq, max_norm, grad_div_dev, guard, skipped, state, ST);
}
int avllm_adamw_step_multi_dev(const avllm_adamw_seg* segs, int32_t nseg, float lr, float b1, float b2, float eps, int32_t step, const float* sumsq,
                               float max_norm, const float* grad_div_dev, const float* guard, float* skipped, const avllm_step_state* state,
                               void* stream) {
    return av_adamw_step_multi_dev(segs, nseg, lr, b1, b2, eps, step, sumsq, max_norm, grad_div_dev, guard, skipped, state, ST);
}
int avllm_step_advance_micro(avllm_step_state* state, const avllm_schedule* sched, void* stream) { return av_step_advance_micro(state, sched, ST); }
int avllm_window_add(float* window, const float* acc, const avllm_step_state* state, void* stream) { return av_window_add(window, acc, state, ST); }
int avllm_lora_pack(const float* A, const float* Bm, int32_t r, int32_t din, int32_t dout, void* A_pad, void* AT_pad, int64_t ld_at,
                    void* B_pad, void* BT_pad, int32_t dtype, void* stream) { return av_lora_pack(A, Bm, r, din, dout, A_pad, AT_pad, ld_at, B_pad, BT_pad, dtype, ST); }
int avllm_lora_merge(void* W, int64_t ldw, int32_t N, int32_t K, const float* A, const float* B, int32_t r, float scale, int32_t dtype,
                     void* stream) { return av_lora_merge(W, ldw, N, K, A, B, r, scale, dtype, ST); }
}
