// Internal launchers (typed stream) behind the C ABI of include/avllm.h.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/avllm.h"

// The current device (0 when the runtime cannot say), as an index below AV_MAX_DEVICES for the launchers' per-device "dynamic LDS limit raised"
// flags, and its CU count (cached per device; 256 when the runtime cannot say): the grid of the persistent kernels.
#define AV_MAX_DEVICES 64
int av_device(int* ncu);
int av_gemm_plan(const avllm_gemm_desc* d, int* kernel);
int av_gemm(const avllm_gemm_desc* d, hipStream_t st);
bool av_gemm_dp_ok(const avllm_gemm_desc* d);                                              // gemm_dp.hip: the calls its kernel takes, and its
int av_gemm_dp(const avllm_gemm_desc* d, hipStream_t st, int dbg, int dev, int ncu);       // launch, for av_gemm alone
int av_gemm_tn(const void* P, long ldp, int I, const void* Q, long ldq, int J, int M, float* out, long ldo,
               float alpha, int dtype, hipStream_t st, uint32_t drop_seed = 0, float drop_p = 0.f, const uint32_t* seed_dev = nullptr);
int av_layernorm(const void* x, const void* w, const void* b, void* y, long rows, int d, float eps, int dtype, hipStream_t st);
int av_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, long rows, int d, float eps, int dtype, hipStream_t st);
int av_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, const void* dres_in, void* dx_out,
                   long rows, int d, int dtype, hipStream_t st);
int av_rope(void* x, long ld, long rows, int T, int heads, int hd, int pos0, float theta, int inverse, int dtype, hipStream_t st);
int av_swiglu_fwd(const void* gu, void* h, long M, int F, int dtype, hipStream_t st);
int av_swiglu_bwd(const void* dh, const void* gu, void* dgu, long M, int F, int dtype, hipStream_t st);
int av_swiglu_bwd_h(const void* dh, const void* gu, void* dgu, void* h, long M, int F, int dtype, hipStream_t st);
// Which kernel an attention call gets (AVLLM_ATTN_<form> of avllm.h): every dispatch below switches on these two
int av_attention_fwd_form(int B, int Tq, int Tk, int hd, int causal, int dtype, int impl);
int av_attention_bwd_form(int hd, int dtype, int impl);
// attention_ref.hip (scalar kernels, delta) and attention_bwd.hip (MFMA backward), reached through av_attention_fwd / av_attention_bwd
int av_attention_fwd_ref(const void* q, const void* k, const void* v, void* o, float* lse, int B, int Tq, int Tk, int H,
                         int hd, long ldq, long ldk, long ldv, long ldo, float scale, int causal, int dtype, hipStream_t st, int G);
int av_attention_delta(const void* o, const void* dout, float* delta, int B, int T, int H, int hd, long ldo, long lddo, int dtype, hipStream_t st);
int av_attention_bwd_ref(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
                         void* dq, void* dk, void* dv, int B, int T, int H, int hd, long ldq, long ldk, long ldv, long lddo,
                         long lddq, long lddk, long lddv, float scale, int causal, int dtype, hipStream_t st, int G);
int av_attention_bwd_mfma(const void* q, const void* k, const void* v, const void* dout, const float* lse, float* delta,
                          void* dq, void* dk, void* dv, int B, int T, int H, int hd, long ldq, long ldk, long ldv, long lddo,
                          long lddq, long lddk, long lddv, float scale, int causal, hipStream_t st, int G, const void* o, long ldo, const float* rope_tab);
bool av_attention_fwd_mxq_ok(int B, int T, int H, int hd, int dtype, int kv_heads);
int av_attention_fwd_mxq(const void* q, const void* k, const void* v, void* oq, long ldoq, void* osc, int B, int T, int H, int hd, long ldq, long ldk,
                         long ldv, float scale, hipStream_t st);
int av_attention_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int Tq, int Tk, int H,
                     int hd, long ldq, long ldk, long ldv, long ldo, float scale, int causal, int dtype, int impl,
                     hipStream_t st, int kv_heads = 0);
int av_attention_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                     void* dq, void* dk, void* dv, float* delta_ws, int B, int T, int H, int hd, long ldq, long ldk,
                     long ldv, long ldo, long lddq, long lddk, long lddv, float scale, int causal, int dtype, int impl,
                     hipStream_t st, int kv_heads = 0, const float* rope_tab = nullptr);
// rope_tab != NULL: dq and dk come out as gradients w.r.t. the PRE-RoPE q/k (inverse rotation applied in the kernels' epilogues)
bool av_attention_bwd_fuses_rope(int dtype, int hd, int impl);
int av_ce_fwd(const void* logits, long ld, const int64_t* labels, int B, int T, int V, float* row_lse, float* loss_sum,
              float* count, int dtype, hipStream_t st);
int av_ce_bwd(const void* logits, long ld, const int64_t* labels, const float* row_lse, const float* count,
              float grad_scale, void* dlogits, int B, int T, int V, int dtype, hipStream_t st);
int av_ce_smooth_fwd(const void* logits, long ld, const int64_t* labels, int B, int T, int V, float eps, float zeta, float* row_lse,
                     float* loss_sum, float* count, float* terms, int dtype, hipStream_t st);
int av_ce_smooth_bwd(const void* logits, long ld, const int64_t* labels, const float* row_lse, const float* count, float grad_scale,
                     float eps, float zeta, void* dlogits, int B, int T, int V, int dtype, hipStream_t st);
int av_argmax_rows(const void* logits, long ld, long rows, int V, int64_t* out, int dtype, hipStream_t st);
int av_sample_rows(const void* logits, long ld, long rows, int V, float temperature, int top_k, float top_p, uint32_t seed,
                   const uint32_t* row_seeds, int step, const int* step_dev, uint8_t* unfinished, long long eos, long long pad,
                   int64_t* out, float* out_logprob, int dtype, hipStream_t st);
int av_row_scores(const void* logits, long ld, long rows, int V, const int64_t* tokens, float temperature, float* out_logprob, float* out_entropy,
                  int logprobs, int dtype, hipStream_t st);
size_t av_beam_topk_workspace_bytes(long rows, int V, int k);
int av_beam_topk(const float* logits, long ld, int B, int nb, int V, const float* beam_scores, int k, float* out_scores, int32_t* out_beams,
                 int64_t* out_tokens, void* ws, size_t ws_bytes, int logprobs, hipStream_t st);
int av_logits_process(const avllm_logits_proc_desc* d, hipStream_t st);
int av_kv_gather_rows(const void* k_src, const void* v_src, int src_rows, long src_T, void* k_dst, void* v_dst, int dst_rows, long dst_T,
                      int layers, int dkv, const int32_t* parent, int t0, int t1, int dtype, hipStream_t st);
int av_embedding(const void* table, const int64_t* ids, void* out, long n, int d, int dtype, hipStream_t st);
int av_cast(const void* src, int sdt, void* dst, int ddt, long n, hipStream_t st);
int av_whisper_im2col1(const float* mel, void* cols, int B, int n_mels, int T, int Kpad, int dtype, hipStream_t st);
int av_whisper_im2col2(const void* h, void* cols, int B, int T, int d, int dtype, hipStream_t st);
int av_clip_patchify(const void* frames, void* cols, int N, int S, int p, int Kpad, int dtype, hipStream_t st, int in_dtype = AV_F32);
int av_clip_cls_rows(const void* class_emb, const void* pos, void* x, int N, int tokens, int d, int dtype, hipStream_t st);
int av_fuse_pool(const void* a, int Ta, const void* v, int Tv, const void* prompt_emb, int P, void* out, int B, int L,
                 int S_out, int D, float fs, int dtype, hipStream_t st);
int av_fuse_pool_bwd(const void* dx, void* da, int Ta, void* dv, int Tv, int P, int B, int L, int S_out, int D, float fs, int dtype, hipStream_t st);
int av_fuse_pool_rows(const void* a, int Ta, const void* v, int Tv, const void* prompt_emb, int P, const int* mode, void* out, int B, int L,
                      int S_out, int D, float fs, int dtype, hipStream_t st);
int av_fuse_pool_rows_bwd(const void* dx, void* da, int Ta, void* dv, int Tv, int P, const int* mode, int B, int L, int S_out, int D, float fs,
                          int dtype, hipStream_t st);
int av_modality_draw(const int* mode_in, int* mode_out, int B, float p_drop_audio, float p_drop_video, uint32_t seed, const uint32_t* seed_dev,
                     hipStream_t st);
int av_gemm_wgrad(const void* dY, long ldy, const void* X, long ldx, int M, int N, int K, float* dW, long ldw, float* db, float alpha, int dtype,
                  hipStream_t st);
int av_gemm_wgrad_acc(const void* dY, long ldy, const void* X, long ldx, int M, int N, int K, float* dW, long ldw, float* db, float alpha, int dtype,
                      hipStream_t st);
int av_adamw_step_dev(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps,
                      float wd, int step, const float* sumsq, float max_norm, const float* grad_div_dev, const float* guard, float* skipped,
                      const avllm_step_state* state, hipStream_t st);
int av_adamw_step_multi_dev(const avllm_adamw_seg* segs, int nseg, float lr, float b1, float b2, float eps, int step, const float* sumsq,
                            float max_norm, const float* grad_div_dev, const float* guard, float* skipped, const avllm_step_state* state,
                            hipStream_t st);
int av_step_advance_micro(avllm_step_state* state, const avllm_schedule* sched, hipStream_t st);
int av_window_add(float* window, const float* acc, const avllm_step_state* state, hipStream_t st);
int av_grad_sumsq_det_multi(const float* const* g, const int64_t* n, int nbuf, float* partials, int nparts, float* sumsq, hipStream_t st);
int av_adamw_step_multi(const avllm_adamw_seg* segs, int nseg, float lr, float b1, float b2, float eps, int step, const float* sumsq, float max_norm,
                        float grad_prescale, const float* guard, float* skipped, const avllm_step_state* state, hipStream_t st);
int av_grad_sumsq(const float* g, long n, float* sumsq, hipStream_t st);
int av_grad_sumsq_det(const float* g, long n, float* partials, int nparts, float* sumsq, hipStream_t st);
int av_adamw_step(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps,
                  float wd, int step, const float* sumsq, float max_norm, float grad_prescale, const float* guard, float* skipped,
                  const avllm_step_state* state, hipStream_t st);
int av_lora_pack(const float* A, const float* Bm, int r, int din, int dout, void* A_pad, void* AT_pad, long ld_at,
                 void* B_pad, void* BT_pad, int dtype, hipStream_t st);
int av_lora_merge(void* W, long ldw, int N, int K, const float* A, const float* B, int r, float scale, int dtype, hipStream_t st);
int av_kv_append(const void* k, const void* v, long ld, void* kc, void* vc, int B, int T, int pos0, int Tmax, int d,
                 int dtype, hipStream_t st);
int av_attention_decode(const void* q, long ldq, const void* kc, const void* vc, void* o, long ldo, int B, int H, int hd,
                        int Tk, int Tmax, float scale, int dtype, hipStream_t st, int G = 1);
int av_attention_decode1(const void* q, long ldq, const void* kc, const void* vc, void* o, long ldo, int B, int H, int hd, int Tk, const int* tk_dev,
                         int Tmax, float scale, int dtype, hipStream_t st, int G);
// fp8 KV cache (kv_fp8.hip; its attention: attention_decode.hip): kq / ke / vq / ve are the code and exponent planes of one layer's K and V images [B, Tmax, dkv] / [B, Tmax, dkv/32]
int av_kv8_append(const void* k, const void* v, long ld, void* kq, void* ke, void* vq, void* ve, int B, int T, int pos0, int Tmax, int dkv, hipStream_t st);
int av_kv8_rope_append(void* qkv, long ld, int B, int H, int Hkv, int hd, const float* rope, int rotate, void* kq, void* ke, void* vq, void* ve, int Tmax,
                       int pos, const int* pos_dev, hipStream_t st);
int av_attention_decode_kv8(const void* q, long ldq, const void* kq, const void* ke, const void* vq, const void* ve, void* o, long ldo, int B, int H, int hd,
                            int Tk, const int* tk_dev, int Tmax, float scale, int G, hipStream_t st);
// shared-prefix single-token attention (attention_decode_shared.hip): R = B group rows; row r attends prefix rows [0, S) of item r / group in the
// B-row cache [B, Tp, dkv], then its own suffix rows [0, Tk + *tk_dev) (clamped to N) of [R, N, dkv].  bf16; ws: av_attention_decode_shared_ws bytes
size_t av_attention_decode_shared_ws(int R, int H, int hd);
int av_attention_decode_shared(const void* q, long ldq, const void* kp, const void* vp, int S, int Tp, const void* ks, const void* vs, int Tk, const int* tk_dev,
                               int N, void* o, long ldo, int R, int group, int H, int hd, float scale, int GQ, void* ws, size_t ws_bytes, hipStream_t st);
int av_attention_decode_shared_kv8(const void* q, long ldq, const void* kpq, const void* kpe, const void* vpq, const void* vpe, int S, int Tp, const void* ksq,
                                   const void* kse, const void* vsq, const void* vse, int Tk, const int* tk_dev, int N, void* o, long ldo, int R, int group, int H,
                                   int hd, float scale, int GQ, void* ws, size_t ws_bytes, hipStream_t st);
int av_kv8_gather_rows(const void* k_src, const void* v_src, int src_rows, long src_T, void* k_dst, void* v_dst, int dst_rows, long dst_T, int layers,
                       int dkv, const int32_t* parent, int t0, int t1, hipStream_t st);
int av_norm_mxq(const void* x, const void* w, const void* b, void* y, float* rstd_out, void* q, long ldq, void* scales, long rows, int d, float eps,
                hipStream_t st);
bool av_lora_batch_supported(int dtype, int R, int nj);
int av_lora_rank3(const void* const* A, const long* lda, const int* K, const void* const* B, const long* ldb, void* const* C, const long* ldc,
                  const uint32_t* seeds, int nj, int M, int R, float alpha, float p, const uint32_t* seed_dev, int shared, int dtype, hipStream_t st);
int av_gemm_tn_multi(const void* Big, long ldb, int NB, const void* const* Small, const long* lds, float* const* out, const long* ldo,
                     const int* col0, const int* ncol, const uint32_t* seeds, int nj, int R, int M, float alpha, float p,
                     const uint32_t* seed_dev, int shared, int dtype, hipStream_t st);
bool av_dec_proj_supported(int dtype, int M, int K, int N, int mode, int hd);
int av_dec_proj(const avllm_dec_proj_desc* d, hipStream_t st);
struct AvRopeScale { float factor = 1.f, low_freq_factor = 1.f, high_freq_factor = 4.f; int orig_ctx = 0; };      // orig_ctx == 0: plain RoPE
int av_rope_table(float* tab, int T, int hd, int pos0, float theta, hipStream_t st, const int* pos_dev = nullptr, AvRopeScale sc = AvRopeScale());
int av_rope_tab(void* x, long ld, long rows, int T, int heads, int hd, const float* tab, int inverse, int dtype, hipStream_t st);
// per-head RMSNorm of the q and k heads + rotary embedding in place (qk_norm.hip); pre / rstd: optional saves for av_qk_norm_bwd; kc / vc:
// cache form (T == 1): rotated k and untouched v go to cache row pos + *pos_dev instead, q stays in x
int av_qk_norm_rope(void* x, long ld, long M, int T, int H, int Hkv, int hd, const void* wq, const void* wk, float eps, const float* tab, void* pre,
                    float* rstd, void* kc, void* vc, int Tmax, int pos, const int* pos_dev, int dtype, hipStream_t st);
int av_qk_norm_bwd(void* dy, long ld, long M, int H, int Hkv, int hd, const void* wq, const void* wk, const void* pre, const float* rstd, int dtype,
                   hipStream_t st);
int av_dropout(const void* x, void* y, long rows, int d, uint32_t seed, float p, int dtype, hipStream_t st, const uint32_t* seed_dev = nullptr);
bool av_lora_dx_masked_supported(int dtype, int N, int r, const long* ldt, const long* ldat, int nj, long ldr, long ldo);
int av_lora_dx_masked(const void* const* T, const long* ldt, const void* const* AT, const long* ldat, const uint32_t* seeds, int nj, int r,
                      const void* R, long ldr, void* out, long ldo, int M, int N, float p, const uint32_t* seed_dev, int dtype, hipStream_t st);
int av_mx_quantize(const void* x, long ldx, int R, int K, void* q, long ldq, void* scales, int layout, int dtype, hipStream_t st);
int av_gemm_f8(const avllm_gemm_f8_desc* d, hipStream_t st);
int av_act_residual(const void* x, const void* r, void* y, long n, int act, int dtype, hipStream_t st);
int av_step_advance(avllm_step_state* state, const avllm_schedule* sched, hipStream_t st);
