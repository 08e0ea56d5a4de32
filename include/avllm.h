/*
 * avllm.h -- C ABI of libavllm.so, the MI355X (gfx950) implementation of the AV->LLM hot path of
 * rishabhjain16/audio-visual-llm `src/clip_whisper`.
 *
 * The reference has no FFI of its own: its seam is the Python class surface
 * (src/clip_whisper/models/clip_whisper_model.py, trainer/clip_whisper_trainer.py).  The entry points
 * below are what a ctypes binding under those classes calls; each cites the reference interface it
 * replaces.  Plain pointers and sizes only: every `const void*`/`void*` is a DEVICE pointer unless the
 * comment says host; `stream` is a hipStream_t passed as void* (NULL = default stream).  All functions
 * are asynchronous on `stream`, return 0 on success or an AVLLM_ERR_* code, and leave a message for
 * avllm_last_error() (thread local).  No function allocates device memory: scratch comes from the
 * caller-provided workspace.
 *
 * dtype: AVLLM_F32 (strict-parity mode, fp32 MFMA) or AVLLM_BF16 (bf16 storage, fp32 accumulate).
 */
#ifndef AVLLM_H
#define AVLLM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define AVLLM_F32 0
#define AVLLM_BF16 1
#define AVLLM_ACT_NONE 0
#define AVLLM_ACT_GELU 1        /* erf GELU  (Whisper, HF:models/whisper/modeling_whisper.py:618-619,:405) */
#define AVLLM_ACT_QUICK_GELU 2  /* x*sigmoid(1.702x) (CLIP, HF:models/clip/modeling_clip.py:346-350) */
#define AVLLM_ACT_SILU 3
#define AVLLM_LORA_PAD 64       /* LoRA rank is stored padded to this many columns */

const char* avllm_last_error(void);
int avllm_version(void);

/* ---------------------------------------------------------------- op level -------------------- */

/* C[M,N] = act(alpha*(A.B^T + A2.B2^T) + bias) + R ; replaces every nn.Linear / F.linear on the path
 * (modality_connector.py:43-44; HF q/k/v/out/fc1/fc2/gate/up/down/lm_head) incl. the peft LoRA add. */
typedef struct avllm_gemm_desc {
    const void* A;  const void* B;      /* A [M,K] row stride lda; B [N,K] row stride ldb (nn.Linear weight) */
    const void* A2; const void* B2;     /* optional second K segment [M,K2] / [N,K2] (LoRA), NULL if K2==0 */
    void* C;                            /* [M,N] row stride ldc */
    const void* bias;                   /* [N] in `dtype`, or NULL */
    const void* R;                      /* residual [M,N] (or [r_mod,N]) in `dtype`, or NULL */
    int64_t lda, ldb, lda2, ldb2, ldc, ldr;
    int32_t M, N, K, K2;                /* K, K2 multiples of 64 */
    int32_t dtype;                      /* of A,B,A2,B2,bias,R (and C unless out_f32) */
    int32_t out_f32;                    /* store C as float even in bf16 mode */
    int32_t act;
    float alpha;
    int32_t r_mod;                      /* >0: residual row = m % r_mod (broadcast position embeddings) */
    int32_t g_in, g_out, g_off;         /* g_in>0: output row = (m/g_in)*g_out + g_off + m%g_in */
    uint32_t drop_seed;                 /* drop_p>0: the product (before +R) is multiplied by the dropout mask */
    float drop_p;                       /*   keep(drop_seed, m*N+n, p)/(1-p)  -- see avllm_dropout */
    uint32_t a_drop_seed;               /* a_drop_p>0: the A operand is dropout(A), mask index m*K+k (bf16, N==64 rank-side GEMM only): */
    float a_drop_p;                     /*   peft's lora_A(dropout(x)) without materialising dropout(x) */
    int32_t n_valid;                    /* N == 64 rank-side GEMM: only rows [0,n_valid) of B are non-zero (rank padded to 64); the other
                                         * output columns are written as zeros without being computed.  0 = all N */
    const uint32_t* seed_dev;           /* optional DEVICE word added to drop_seed / a_drop_seed at run time (see avllm_step_state) */
} avllm_gemm_desc;
int avllm_gemm(const avllm_gemm_desc* d, void* stream);
/* Which kernel avllm_gemm runs for a call: *kernel = one of the ids below, or the error avllm_gemm itself would return.  Pure host code (no
 * device needed, no operand read: pointers count for their alignment only); the descriptor and the knobs "GEMM_VARIANT" / "NARROW_EPILOGUE"
 * decide.  DESIGN.md "Which GEMM kernel a call gets" lists the conditions. */
enum { AVLLM_GEMM_SMALLM, AVLLM_GEMM_SKINNY64, AVLLM_GEMM_128, AVLLM_GEMM_RING, AVLLM_GEMM_H16, AVLLM_GEMM_HP16, AVLLM_GEMM_W4, AVLLM_GEMM_WP4,
       AVLLM_GEMM_DP, AVLLM_GEMM_F32, AVLLM_GEMM_KERNELS };
int avllm_gemm_plan(const avllm_gemm_desc* d, int32_t* kernel);
/* A/B testing only: avllm_set_knob("GEMM_VARIANT", v).  Forces one bf16 tiling (<= 0 = automatic choice): 1 = 128x128, 2 = 256x128 ring, 5 / 6 =
 * 256x256 with 16 waves (one-shot / persistent), 7 / 8 = 256x256 with 4 waves (one-shot / persistent: the default for every lean-epilogue call on a
 * chip-filling grid), 9 = 256x128 persistent with two workgroups per CU (csrc/gemm_dp.hip).  Any forced variant switches the M <= 16 kernel off; the
 * N == 64 rank-side kernel and the fp32 kernel keep their calls.  A call the forced variant cannot take (M <= 128; 7 / 8 / 9: K + K2 < 128; 8 / 9: an
 * epilogue that is not lean) runs on the 128x128 kernel, not on the automatic choice; 5 on operands of 2^32 elements or more is an error. */
int avllm_set_gemm_variant(int v);
/* A/B testing only: the library's experiment switches live in ONE table that is filled once per process from the environment
 * (AVLLM_<NAME>) and changed afterwards only through this call.  Names: "DECODE_FUSED" (0 = general 10-launch decode layer),
 * "DEC_AL" (force an activation-load form of avllm_dec_proj: 2 | 4), "LORA_UNBATCHED" (1 = one launch per adapter), "F8_UNFUSED_QUANT"
 * (1 = separate quantiser passes), "F8_FAST" (0 = reference-grade fp8 GEMM), "ATTN_SHORT" (0 = general attention kernel for T <= 272),
 * "NARROW_EPILOGUE", "TN_CHUNK", "GEMM_VARIANT" (avllm_set_gemm_variant above), "GEMM_GW" (tile-column group width of the persistent GEMM's walk on tall shapes: 0 = row-major walk,
 * n = groups of n columns), "GEMM_DBG" (only read by builds made with -DAVLLM_EXPERIMENT_KNOBS), "SHARED_SPLIT" (A/B testing: forces the launch form
 * of avllm_attention_decode_shared: 1 .. 16 = two launches with that many prefix slices, -1 = one launch; 0 = its own choice).  Unknown name -> error. */
int avllm_set_knob(const char* name, int32_t value);
int avllm_get_knob(const char* name, int32_t* value);      /* the value in force (to put it back after an A/B block) */

/* out[I,J] (f32, row stride ldo) += alpha * sum_m P[m,i]*Q[m,j]; LoRA dA/dB (autograd of peft lora.Linear) */
int avllm_gemm_tn(const void* P, int64_t ldp, int32_t I, const void* Q, int64_t ldq, int32_t J, int32_t M,
                  float* out, int64_t ldo, float alpha, int32_t dtype, void* stream);
/* same, with dropout(seed,p) applied on the fly to the WIDE operand (mask index m*width+col; bf16 MFMA path only) */
int avllm_gemm_tn_drop(const void* P, int64_t ldp, int32_t I, const void* Q, int64_t ldq, int32_t J, int32_t M,
                       float* out, int64_t ldo, float alpha, uint32_t drop_seed, float drop_p, int32_t dtype, void* stream);

/* Weight gradient of a Linear (autograd of nn.Linear: SimpleModalityConnector.linear, modality_connector.py:25-44, reached by the loss when
 * the connectors train, clip_whisper_model.py:1096-1106,1136-1146):  dW[N,K] (f32, row stride ldw, OVERWRITTEN) = alpha * dY^T . X with
 * dY [M,N] (row stride ldy) and X [M,K] (row stride ldx), both row-major over the reduction index m and of `dtype`; db[N] (f32, may be NULL)
 * = alpha * sum_m dY[m,n].  One workgroup owns an output tile for the whole of M and db is summed in a fixed order: no float atomics, two
 * launches are bit-identical.  bf16: both operands through LDS, MFMA fragments by transposed LDS reads, fp32 accumulators; fp32: a scalar
 * kernel (parity mode).  Any M >= 1; N, K, ldy, ldx must be multiples of 8 and dY, X 16-byte aligned (anything else is refused). */
int avllm_gemm_wgrad(const void* dY, int64_t ldy, const void* X, int64_t ldx, int32_t M, int32_t N, int32_t K, float* dW, int64_t ldw,
                     float* db, float alpha, int32_t dtype, void* stream);
/* The accumulating form (gradient accumulation over micro-batches):  dW[n,k] = dW[n,k] + alpha * sum_m dY[m,n] X[m,k]  and
 * db[n] = db[n] + alpha * sum_m dY[m,n].  The same kernels and K-loop with another epilogue: the cell's prior value is read once, after the
 * reduction, and added once to the ROUNDED product alpha * acc, in fp32 (two roundings, never one fma).  One workgroup still owns its tile for the
 * whole of M: no atomics, two launches from the same prior value are bit-identical, and onto a zeroed dW / db the result is avllm_gemm_wgrad's
 * bits.  Cells of a row past K (ldw > K) are neither read nor written.  Arguments and refusals are those of avllm_gemm_wgrad. */
int avllm_gemm_wgrad_acc(const void* dY, int64_t ldy, const void* X, int64_t ldx, int32_t M, int32_t N, int32_t K, float* dW, int64_t ldw,
                         float* db, float alpha, int32_t dtype, void* stream);

/* The q / k / v adapters of one decoder layer batched (bf16, rank <= 16, 1..3 adapters; peft lora.Linear on q_proj, k_proj, v_proj,
 * clip_whisper_model.py:961-1005).  Rank-side products C_j[M,64] = alpha * A_j[M,K_j] B_j[:R,K_j]^T:
 * shared != 0: every adapter reads A[0] through its own dropout mask (forward lora_A(dropout(x)); mask index m*K+k, seeds[j] (+ *seed_dev),
 * needs lda == K); shared == 0: adapter j reads A[j] (backward dt_j = s dy_j B_j; no mask).  K_j % 256 == 0.
 * What B must be: the kernel is not told R.  It reads SIXTEEN rows of every B_j (row stride ldb[j]) and writes all sixteen products, so B_j
 * must have at least 16 readable rows and rows R..15 must be zeros: avllm_lora_pack's padded image.  A true [R, K] tensor with R < 16 is an
 * out-of-bounds read.  What is then promised: every one of the 64 columns of C_j is written, columns >= R as zeros (R..15 are the products
 * with B's zero rows, 16..63 are stored zeros: the K2 segment of the projection GEMM). */
int avllm_lora_rank3(const void* const* A, const int64_t* lda, const int32_t* K, const void* const* B, const int64_t* ldb, void* const* C,
                     const int64_t* ldc, const uint32_t* seeds, int32_t nj, int32_t M, int32_t R, float alpha, float p,
                     const uint32_t* seed_dev, int32_t shared, int32_t dtype, void* stream);
/* Reductions over tokens for the same adapters (fp32 atomic accumulation into out_j, as avllm_gemm_tn):
 * shared != 0: out_j[R, NB] += alpha * Small_j^T . dropout_j(Big)            (dA_j; Big [M, NB] read once)
 * shared == 0: out_j[ncol_j, R] += alpha * Big[:, col0_j:+ncol_j]^T . Small_j (dB_j; the ranges tile Big's NB columns in 128-column units) */
int avllm_gemm_tn_multi(const void* Big, int64_t ldb, int32_t NB, const void* const* Small, const int64_t* lds, float* const* out,
                        const int64_t* ldo, const int32_t* col0, const int32_t* ncol, const uint32_t* seeds, int32_t nj, int32_t R,
                        int32_t M, float alpha, float p, const uint32_t* seed_dev, int32_t shared, int32_t dtype, void* stream);

/* Input gradient of up to three LoRA adapters that share one input x, under lora_dropout, in one pass (bf16):
 *   out[M,N] = R[M,N] + sum_j keep(seeds[j] (+ *seed_dev), m*N+n, p)/(1-p) * (T_j[M,r] . A_j[r,N])
 * autograd of peft's lora_B(lora_A(dropout(x))) w.r.t. x (clip_whisper_model.py:961-1005).  T_j [M, >= 32 cols] (zeros past the rank, row
 * stride ldt[j]); AT_j = the padded transposed image of A_j [N, >= 32 cols] (avllm_lora_pack's AT_pad, row stride ldat[j]); T / AT / ldt /
 * ldat / seeds are HOST arrays of nj <= 3 entries; out may alias R.  N % 128 == 0, r <= 32. */
int avllm_lora_dx_masked(const void* const* T, const int64_t* ldt, const void* const* AT, const int64_t* ldat, const uint32_t* seeds,
                         int32_t nj, int32_t r, const void* R, int64_t ldr, void* out, int64_t ldo, int32_t M, int32_t N, float p,
                         const uint32_t* seed_dev, int32_t dtype, void* stream);

/* ---- block-scaled fp8 (OCP MX: e4m3 elements + one E8M0 scale per 32 K elements; BASELINE config 5, "fp8 MFMA").  The reference has no
 * such mode (clip_whisper_model.py:164: only use_fp16); these entry points give nn.Linear's y = act(x W^T + b) + R on
 * v_mfma_scale_f32_16x16x128_f8f6f4 with fp32 accumulation, bf16 output.
 * avllm_mx_quantize: x [R,K] (bf16 or f32, row stride ldx) -> q uint8 [R,K] (row stride ldq bytes) + the scale image of
 * avllm_mx_scale_bytes(R,K) bytes.  layout 0 = activation side, 1 = weight side (csrc/fp8.hip, "Formats").  layout 2 = the decode side:
 * `scales` is the plain exponent matrix uint8 [R, K/32] (E8M0, biased by 127, row-major: R*K/32 bytes), the E8 of avllm_dec_proj. */
size_t avllm_mx_scale_bytes(int32_t R, int32_t K);
int avllm_mx_quantize(const void* x, int64_t ldx, int32_t R, int32_t K, void* q, int64_t ldq, void* scales, int32_t layout, int32_t dtype,
                      void* stream);
/* OCP MXFP4 weight images of the token step (avllm_dec_proj's fp4 form): x [R,K] (bf16 or f32, row stride ldx, K % 32 == 0) -> q uint8
 * [R, K/2] (row stride ldq bytes, ldq % 16 == 0), two e2m1 codes per byte with element 2i in the low nibble, and exps uint8 [R, K/32]
 * row-major, E8M0 biased by 127.  Rule (OCP MX v1.0, emax = 2): e = floor(log2(amax of the 32-block)) - 2 clamped to [-127, 127] (all-zero
 * block: -127); codes = x * 2^-e rounded to nearest even onto {0, 0.5, 1, 1.5, 2, 3, 4, 6}, saturated at +-6; bit 3 = sign. */
int avllm_mx4_quantize(const void* x, int64_t ldx, int32_t R, int32_t K, void* q, int64_t ldq, void* exps, int32_t dtype, void* stream);
typedef struct avllm_gemm_f8_desc {
    const void* A;  const void* SA;     /* activations: q [M,K] (layout 0 scales) */
    const void* B;  const void* SB;     /* weights:     q [N,K] (layout 1 scales), nn.Linear orientation */
    void* C;                            /* bf16 [M,N] */
    const void* bias;                   /* bf16 [N] or NULL */
    const void* R;                      /* bf16 residual [M,N] or NULL (may alias C) */
    int64_t lda, ldb, ldc, ldr;
    int32_t M, N, K;                    /* K % 128 == 0 */
    int32_t act;
    /* Quantised output (the activation of the NEXT fp8 projection, e.g. fc1 -> fc2): when Cq != NULL the result act(A.B^T + bias) is
     * block-scaled to e4m3 in the epilogue, straight from the fp32 accumulators -- codes uint8 [M,N] (row stride ldcq bytes) + the layout-0
     * scale image of avllm_mx_scale_bytes(M,N) bytes in SCq -- and the bf16 C is NOT written (C may be NULL; R must be NULL; N % 128 == 0:
     * the image holds N / 128 planes).
     * Only the persistent kernel implements it: AVLLM_ERR_UNSUPPORTED for calls it does not take (avllm_gemm_f8_takes_quantised_output). */
    void* Cq; void* SCq;
    int64_t ldcq;
} avllm_gemm_f8_desc;
int avllm_gemm_f8_takes_quantised_output(const avllm_gemm_f8_desc* d);
/* 1 where avllm_gemm_f8 runs the call on the persistent 256x256 kernel, 0 where the reference-grade kernel takes it (or, with Cq, refuses). */
int avllm_gemm_f8_takes_fast(const avllm_gemm_f8_desc* d);
int avllm_gemm_f8(const avllm_gemm_f8_desc* d, void* stream);
/* nn.LayerNorm (b != NULL; HF whisper / clip encoder layers) or LlamaRMSNorm (b == NULL) of bf16 rows with the result block-scaled to e4m3 in
 * the same pass: q uint8 [rows, d] (row stride ldq) + the layout-0 scale image, ready as the A operand of avllm_gemm_f8.  y (bf16 copy of the
 * normalised rows) and rstd_out (RMSNorm's per-row 1/rms, saved for the backward) are optional.  d % 128 == 0, d <= 8192. */
int avllm_norm_mxq(const void* x, const void* w, const void* b, void* y, float* rstd_out, void* q, int64_t ldq, void* scales, int64_t rows,
                   int32_t d, float eps, void* stream);

/* Per-step scalars kept in DEVICE memory so that a training step is the same launch sequence every time and can be captured in a
 * hipGraph (trainer/clip_whisper_trainer.py:433-490 recomputes them on the host each step: scheduler.step() :464, the optimizer's
 * step count, torch's dropout RNG).  avllm_step_advance is a one-thread kernel: step += 1, then
 *   lr           = cosine schedule of _setup_optimizer :210-230 at (step-1): base_lr*(1+cos(pi*s/total))/2, or linear warm-up over
 *                  warmup_steps followed by the cosine over the remaining steps (transformers get_cosine_schedule_with_warmup)
 *   bc1, bc2_sqrt = 1-beta1^step, sqrt(1-beta2^step)                           (torch.optim.AdamW bias corrections)
 *   dropout_seed = (step+skipped)*0x9E3779B1 + rank*0x85EBCA6B + 12345         (this step's LoRA dropout mask seed)
 * Consumers: avllm_llama.dropout_seed_dev (-> &state->dropout_seed), avllm_adamw_step(state). */
typedef struct avllm_step_state {
    uint32_t step;                      /* optimizer steps started (1-based after the first advance) */
    uint32_t dropout_seed;
    float lr, bc1, bc2_sqrt;
    float skipped;                      /* steps whose update was skipped by the non-finite guard (see avllm_adamw_step) */
    uint32_t reserved[2];               /* [0]: micro-steps of the open gradient-accumulation window (avllm_step_advance_micro); [1]: unused */
} avllm_step_state;
typedef struct avllm_schedule {
    float base_lr, beta1, beta2;
    int32_t warmup_steps, total_steps;
    uint32_t rank;
} avllm_schedule;
int avllm_step_advance(avllm_step_state* state_dev, const avllm_schedule* sched, void* stream);
/* Gradient accumulation: a window of N micro-batches is ONE optimizer step on their concatenation.  The micro-step form of the advance, a
 * one-thread kernel run at the top of every micro-step; micro = state->reserved[0] counts the micro-steps since the last optimizer step:
 *   micro == 0:  step, lr, bc1, bc2_sqrt advance exactly as in avllm_step_advance; otherwise they stay
 *   any micro:   dropout_seed = (step+skipped)*0x9E3779B1 + rank*0x85EBCA6B + 12345 + micro * AVLLM_MICRO_SEED_STRIDE   (mod 2^32)
 *                -- micro-step 0 keeps avllm_step_advance's seed; every micro-batch of a window, on every rank, draws its own LoRA dropout
 *                masks and modality modes
 *   then         reserved[0] = micro + 1
 * The window's closing optimizer launch (avllm_adamw_step_dev / avllm_adamw_step_multi_dev) sets reserved[0] back to 0, on a taken and on a
 * skipped window alike. */
#define AVLLM_MICRO_SEED_STRIDE 0xC2B2AE35u   /* odd: micro -> micro * stride is a bijection of the 32-bit seeds */
int avllm_step_advance_micro(avllm_step_state* state_dev, const avllm_schedule* sched, void* stream);
/* The window's [loss_sum, count] in device memory: window[0] += acc[0], then window[1] += acc[1] (acc = the micro-step's [loss_sum, count]),
 * by one thread in that order; on the first micro-step of a window (state_dev->reserved[0] <= 1, i.e. right after its advance) the two words
 * are overwritten instead.  No host sync. */
int avllm_window_add(float* window, const float* acc, const avllm_step_state* state_dev, void* stream);

/* Sequence operators of the non-default connectors (modality_connector.py:111-380), activations token-major [B, T, C]:
 * im2col for nn.Conv1d(kernel_size 3, padding 1, stride 1 | 2): cols [B * Tout, 3 C], column kw * C + c = x[b, stride t' + kw - 1, c] (zero outside
 * the sequence), Tout = (T - 1) / stride + 1; the convolution is then avllm_gemm with the weight reshaped to [out, kw * C + c]. */
int avllm_im2col_k3(const void* x, void* cols, int32_t B, int32_t T, int32_t C, int32_t stride, int32_t dtype, void* stream);
/* nn.GroupNorm(groups, C) of the [B, C, T] view of x [B, T, C]: mean / variance over (T, C / groups) per (item, group), affine w, b [C],
 * then act (AVLLM_ACT_*).  (C / groups) % 8 == 0. */
int avllm_groupnorm_tokens(const void* x, const void* w, const void* b, void* y, int32_t B, int32_t T, int32_t C, int32_t groups,
                           float eps, int32_t act, int32_t dtype, void* stream);

/* nn.LayerNorm (HF whisper :379-413, clip :362-384) */
int avllm_layernorm(const void* x, const void* w, const void* b, void* y, int64_t rows, int32_t d, float eps,
                    int32_t dtype, void* stream);
/* LlamaRMSNorm fwd (HF:models/llama/modeling_llama.py:62-67); rstd [rows] optional */
int avllm_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int64_t rows, int32_t d, float eps,
                      int32_t dtype, void* stream);
/* dx_out = dres_in + d(rmsnorm)/dx . dy   (dres_in may be NULL, dx_out may alias dres_in) */
int avllm_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, const void* dres_in,
                      void* dx_out, int64_t rows, int32_t d, int32_t dtype, void* stream);
/* rotary embedding in place on [rows = B*T, heads, hd] slices (row stride ld elements); position = pos0 + row % T;
 * inverse=1 applies the transpose rotation (backward).  HF:models/llama/modeling_llama.py:129-160 */
int avllm_rope(void* x, int64_t ld, int64_t rows, int32_t T, int32_t heads, int32_t hd, int32_t pos0, float theta,
               int32_t inverse, int32_t dtype, void* stream);
/* The same rotation from a cos/sin table, the form the model runs (one table per call instead of powf/cosf/sinf per element and layer):
 * avllm_rope_table fills tab [T][hd/2][2] = (cos, sin) of (pos0 (+ *pos_dev, optional device word) + t) * inv_freq_i in fp32.  orig_ctx > 0
 * applies HF's "llama3" frequency rule (modeling_rope_utils.py _compute_llama3_parameters) with factor / low_freq_factor /
 * high_freq_factor; orig_ctx == 0 is plain RoPE and ignores them.  avllm_rope_tab rotates x in place with row r reading table row r % T. */
int avllm_rope_table(float* tab, int32_t T, int32_t hd, int32_t pos0, float theta, const int32_t* pos_dev, float factor,
                     float low_freq_factor, float high_freq_factor, int32_t orig_ctx, void* stream);
int avllm_rope_tab(void* x, int64_t ld, int64_t rows, int32_t T, int32_t heads, int32_t hd, const float* tab, int32_t inverse,
                   int32_t dtype, void* stream);
/* h = silu(g)*u with gu = [g | u] ([M,2F]); HF:models/llama/modeling_llama.py:175 */
int avllm_swiglu_fwd(const void* gu, void* h, int64_t M, int32_t F, int32_t dtype, void* stream);
int avllm_swiglu_bwd(const void* dh, const void* gu, void* dgu, int64_t M, int32_t F, int32_t dtype, void* stream);
/* avllm_swiglu_bwd that also writes h [M,F] = silu(g) * u in the same pass over gu (what avllm_swiglu_fwd wrote, bit for bit): the backward
 * pass of a down_proj adapter needs the MLP's hidden activation, which the training workspace does not keep per layer. */
int avllm_swiglu_bwd_h(const void* dh, const void* gu, void* dgu, void* h, int64_t M, int32_t F, int32_t dtype, void* stream);
/* softmax(QK^T*scale [+causal]) V.  q/k/v/o: row = token (b*T+t), head h at column h*hd; row strides in elements.
 * lse [B,H,Tq] (natural log) optional.  impl 0 = MFMA flash kernel (bf16 only), 1 = reference-grade scalar kernel.
 * kv_heads (0 = H): grouped-query attention, k/v (and dk/dv) hold kv_heads heads and query head h reads head h/(H/kv_heads)
 * (HF repeat_kv, models/llama/modeling_llama.py:203-212).
 * HF eager_attention_forward: whisper :215-238, clip :259-277, llama sdpa path. */
int avllm_attention_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int32_t B, int32_t Tq,
                        int32_t Tk, int32_t H, int32_t hd, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                        float scale, int32_t causal, int32_t dtype, int32_t impl, int32_t kv_heads, void* stream);
int avllm_attention_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                        const float* lse, void* dq, void* dk, void* dv, float* delta_ws, int32_t B, int32_t T,
                        int32_t H, int32_t hd, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddq,
                        int64_t lddk, int64_t lddv, float scale, int32_t causal, int32_t dtype, int32_t impl,
                        int32_t kv_heads, void* stream);
/* avllm_attention_bwd with the inverse rotary embedding fused into dq | dk (the form the bf16 train step runs): rope_tab [T][hd/2][2] from
 * avllm_rope_table; the gradients leave with respect to the PRE-RoPE q and k, as avllm_attention_bwd followed by avllm_rope_tab(inverse = 1)
 * on dq and dk.  Only the bf16 MFMA kernels (impl 0, head_dim 64 / 128) fuse it: any other form with a table is refused (argument error).  NULL = no rotation. */
int avllm_attention_bwd_rope(const void* q, const void* k, const void* v, const void* o, const void* dout,
                             const float* lse, void* dq, void* dk, void* dv, float* delta_ws, int32_t B, int32_t T,
                             int32_t H, int32_t hd, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddq,
                             int64_t lddk, int64_t lddv, float scale, int32_t causal, int32_t dtype, int32_t impl,
                             int32_t kv_heads, const float* rope_tab, void* stream);
/* Which kernel avllm_attention_fwd / avllm_attention_bwd run for a call: *fwd_form and *bwd_form = one of the ids below (*bwd_form = -1 where
 * Tq != Tk: the backward takes one T).  Pure host code, no device needed; the arguments and the knob "ATTN_SHORT" (0 = short non-causal
 * sequences go to the general kernel) decide.  REF = the scalar kernels (fp32 storage, impl 1, head dims other than 64 and 128); SHORT13X7 /
 * SHORT17X9 = the one-pass kernel of non-causal self-attention at head_dim 64, T <= 208 / <= 272 (B <= 65535); MFMA64X4 / MFMA128X4 = the flash
 * kernels.  The backward has no short form.  avllm_attention_fwd_mxq_ok: 1 where avllm_attention_fwd_mxq takes the call (a short form, no
 * grouped queries, H * hd a multiple of 128); avllm_attention_bwd_fuses_rope: 1 where avllm_attention_bwd_rope takes a table (an MFMA form). */
enum { AVLLM_ATTN_REF, AVLLM_ATTN_SHORT13X7, AVLLM_ATTN_SHORT17X9, AVLLM_ATTN_MFMA64X4, AVLLM_ATTN_MFMA128X4, AVLLM_ATTN_FORMS };
int avllm_attention_plan(int32_t B, int32_t Tq, int32_t Tk, int32_t H, int32_t hd, int32_t causal, int32_t dtype, int32_t impl, int32_t kv_heads,
                         int32_t* fwd_form, int32_t* bwd_form);
int avllm_attention_fwd_mxq_ok(int32_t B, int32_t T, int32_t H, int32_t hd, int32_t dtype, int32_t kv_heads);
int avllm_attention_bwd_fuses_rope(int32_t dtype, int32_t hd, int32_t impl);
/* shifted causal-LM cross entropy (HF:loss/loss_utils.py:49-71): row (b,t) is scored against labels[b,t+1],
 * ignore_index -100 and the last position.  loss_sum/count are ACCUMULATED (zero them first). row_lse [B*T]. */
int avllm_ce_fwd(const void* logits, int64_t ld, const int64_t* labels, int32_t B, int32_t T, int32_t V,
                 float* row_lse, float* loss_sum, float* count, int32_t dtype, void* stream);
/* The same attention for short non-causal sequences (T <= 272, head_dim 64, bf16: the CLIP towers) with the OUTPUT block-scaled to e4m3 in the
 * kernel's epilogue: codes oq [B*T, ldoq] + the layout-0 scale image of an avllm_gemm_f8 A operand (avllm_mx_scale_bytes(B*T, H*hd) bytes),
 * bit-identical to avllm_mx_quantize of the bf16 output.  Used by the fp8 encoders: the bf16 attention output is never written. */
int avllm_attention_fwd_mxq(const void* q, const void* k, const void* v, void* oq, int64_t ldoq, void* scales, int32_t B, int32_t T, int32_t H,
                            int32_t hd, int64_t ldq, int64_t ldk, int64_t ldv, float scale, void* stream);
/* dlogits = (softmax - onehot) * (grad_scale / *count) for scored rows, 0 elsewhere (may alias logits) */
int avllm_ce_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* row_lse, const float* count,
                 float grad_scale, void* dlogits, int32_t B, int32_t T, int32_t V, int32_t dtype, void* stream);
/* The same cross entropy with label smoothing eps = label_smoothing and the auxiliary z-loss zeta = z_loss (PaLM).  Scoring, shift and ld rules
 * are those of avllm_ce_fwd / avllm_ce_bwd.  For a scored row with logits x over the V real columns (never the padding up to ld),
 * lse = log sum_v exp x_v, p = exp(x - lse) and target y:
 *     nll = lse - x_y,   u = lse - (1/V) sum_v x_v,   q = lse^2,   l = (1 - eps) nll + eps u + zeta q,   loss = sum_scored l / count,
 *     d l / d x_v = (1 + 2 zeta lse) p_v - (1 - eps) [v = y] - eps / V.
 * The eps part is F.cross_entropy(label_smoothing = eps).  0 <= eps < 1 and zeta >= 0, both finite; anything else is AV_ERR_ARG.
 * fwd: row_lse [B*T] written for every row; l is ADDED onto *loss_sum and 1 onto *count per scored row (zero them first); terms (optional,
 * [3], accumulated too) receives the raw sums of nll, u and q, so that a perplexity comparable across eps can be logged.  The row's logits are
 * read once: their plain fp32 sum is gathered in the pass that forms lse.
 * bwd: dlogits = d l / d x * (grad_scale / *count) on scored rows, 0 elsewhere and everywhere when *count == 0; may alias logits; columns >= V
 * are not touched.  With eps = zeta = 0 both give the bits of avllm_ce_fwd / avllm_ce_bwd for row_lse, count and dlogits (loss_sum up to the
 * order of the float atomics). */
int avllm_ce_smooth_fwd(const void* logits, int64_t ld, const int64_t* labels, int32_t B, int32_t T, int32_t V,
                        float label_smoothing, float z_loss, float* row_lse, float* loss_sum, float* count,
                        float* terms /* [3], optional, accumulated */, int32_t dtype, void* stream);
int avllm_ce_smooth_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* row_lse, const float* count,
                        float grad_scale, float label_smoothing, float z_loss, void* dlogits,
                        int32_t B, int32_t T, int32_t V, int32_t dtype, void* stream);
int avllm_argmax_rows(const void* logits, int64_t ld, int64_t rows, int32_t V, int64_t* out, int32_t dtype, void* stream);
/* One sampled token per row (GenerationMixin with do_sample=True, clip_whisper_model.py:1326-1340): HF's TemperatureLogitsWarper
 * (logits / temperature), TopKLogitsWarper (top_k > 0: keys below the k-th largest scaled logit dropped, ties kept; 0 = off) and
 * TopPLogitsWarper (top_p < 1: in descending order, the shortest prefix whose tail mass is <= 1 - top_p, plus every token whose scaled logit
 * equals that of the last kept one), then an inverse-CDF draw over the kept tokens in vocabulary-index order with the uniform
 * u = hash(seed + (row_seeds ? row_seeds[r] : 0), step + (step_dev ? *step_dev : 0)): a row's token depends on its logits, its seed and the
 * step only.  top_k == 1 is avllm_argmax_rows exactly.  unfinished (optional, one byte per row): rows with 0 get pad; a row that draws eos
 * (eos >= 0) is cleared.  temperature > 0, 0 < top_p <= 1, top_k >= 0, V <= 524288; deterministic (integer reductions only). */
int avllm_sample_rows(const void* logits, int64_t ld, int64_t rows, int32_t V, float temperature, int32_t top_k, float top_p, uint32_t seed,
                      const uint32_t* row_seeds, int32_t step, const int32_t* step_dev, uint8_t* unfinished, int64_t eos, int64_t pad,
                      int64_t* out, int32_t dtype, void* stream);
/* avllm_sample_rows that also returns the score of each draw (generate(do_sample=True, return_token_scores=True); HF's
 * compute_transition_scores of a sampled token): out_logprob [rows] (f32) = the log-probability of the drawn token under the distribution
 * it was drawn from, i.e. after temperature, top-k and top-p, renormalised over the kept set: (x_id / temperature - max) - log(kept mass).
 * 0 where the kernel returns the argmax with probability one (top_k == 1, an infinite maximum) and for finished rows, which get pad.
 * Tokens are those of avllm_sample_rows for the same arguments; out_logprob == NULL is avllm_sample_rows exactly. */
int avllm_sample_rows_scored(const void* logits, int64_t ld, int64_t rows, int32_t V, float temperature, int32_t top_k, float top_p, uint32_t seed,
                             const uint32_t* row_seeds, int32_t step, const int32_t* step_dev, uint8_t* unfinished, int64_t eos, int64_t pad,
                             int64_t* out, float* out_logprob, int32_t dtype, void* stream);
/* Token scores (generate(return_token_scores=True); HF's output_scores / compute_transition_scores(normalize_logits=True), transformers
 * generation/utils.py): for each row of f32 logits [rows, V] (row stride ld >= V), with y = logits[r] / temperature and
 * lse = log(sum_v exp(y[v])): out_logprob[r] = y[tokens[r]] - lse and out_entropy[r] = lse - sum_v softmax(y)[v] * y[v], the entropy of
 * the row in nats (>= 0).  One pass over the row, one workgroup per row, deterministic (no atomics).  tokens: int64 [rows], clamped to
 * [0, V); NULL: out_logprob[r] = -lse.  out_logprob or out_entropy may be NULL (not both).  Entries of -inf (tokens banned by
 * avllm_logits_process) carry probability 0 in both sums; a chosen token that is -inf scores -inf; a row of nothing but -inf is NOT
 * refused and gives NaN in both outputs.  temperature > 0; V <= 524288; dtype must be AVLLM_F32 (bf16: AV_ERR_UNSUPPORTED). */
int avllm_row_scores(const void* logits, int64_t ld, int64_t rows, int32_t V, const int64_t* tokens, float temperature, float* out_logprob,
                     float* out_entropy, int32_t dtype, void* stream);
/* avllm_row_scores for rows that are log-probabilities already (beam search after avllm_logits_process with log_softmax = 1, the rows
 * avllm_beam_topk_logprobs selects from): nothing is normalised.  out_logprob[r] = logprobs[r][tokens[r]] bit for bit (0 with tokens ==
 * NULL) and out_entropy[r] = -sum_v exp(x[v]) * x[v] over the entries above -inf (0 for a row of nothing but -inf). */
int avllm_row_scores_logprobs(const void* logprobs, int64_t ld, int64_t rows, int32_t V, const int64_t* tokens, float* out_logprob,
                              float* out_entropy, int32_t dtype, void* stream);
/* Beam-search candidate selection (GenerationMixin._beam_search with num_beams > 1, clip_whisper_model.py:1326-1340; transformers
 * generation/utils.py `log_softmax` + `_get_top_k_continuations`).  logits: f32 rows r = b*num_beams + j of length V, row stride ld;
 * beam_scores: f32 [B*num_beams] running sums of log-probabilities (-1e9 and -inf allowed).  For each batch item b, the k best of
 * score(j, v) = beam_scores[r] + ((logits[r][v] - max_r) - log(sum exp(logits[r] - max_r))) (torch.log_softmax in fp32) over all
 * num_beams*V pairs, sorted by score descending; equal scores go to the lower flat index j*V + v first.  A row contributes only its k
 * largest raw logits (equal logits: lower index first).  Outputs [B, k]: out_scores (f32), out_beams (j, int32), out_tokens (v, int64).
 * 1 <= num_beams <= 16, 1 <= k <= 32, k <= num_beams*V, otherwise AV_ERR_ARG.  ws: device scratch of at least
 * avllm_beam_topk_workspace_bytes(B*num_beams, V, k) bytes.  Two launches; deterministic. */
size_t avllm_beam_topk_workspace_bytes(int64_t rows, int32_t V, int32_t k);
int avllm_beam_topk(const float* logits, int64_t ld, int32_t B, int32_t num_beams, int32_t V, const float* beam_scores, int32_t k,
                    float* out_scores, int32_t* out_beams, int64_t* out_tokens, void* ws, size_t ws_bytes, void* stream);
/* avllm_beam_topk for rows that are log-probabilities already (avllm_logits_process with log_softmax = 1): score(j, v) =
 * beam_scores[r] + logprobs[r][v], everything else as above.  Entries of -inf (banned tokens) order below every finite score, so one is
 * returned only when an item has fewer than k finite candidates. */
int avllm_beam_topk_logprobs(const float* logprobs, int64_t ld, int32_t B, int32_t num_beams, int32_t V, const float* beam_scores, int32_t k,
                             float* out_scores, int32_t* out_beams, int64_t* out_tokens, void* ws, size_t ws_bytes, void* stream);
/* The logits processors of `self.llm.generate(**gen_kwargs)` (clip_whisper_model.py:1324-1340) for repetition_penalty, no_repeat_ngram_size
 * and min_new_tokens, in place on scores [rows, V] (f32 or bf16, row stride ld) before avllm_argmax_rows / avllm_sample_rows /
 * avllm_beam_topk_logprobs, in GenerationMixin._get_logits_processor's order.  history: int64 [rows, ldh] on the device, row r's first
 * n = cur + (cur_dev ? *cur_dev : 0) entries are its generated tokens (with inputs_embeds HF's processors see nothing else); entries
 * outside [0, V) are ignored.
 *   RepetitionPenaltyLogitsProcessor(p), p > 0, off at 1: every distinct token t of the history gets s[t] < 0 ? s[t] * p : s[t] / p
 *     (IEEE division), computed once from the unprocessed score however often t occurs.
 *   NoRepeatNGramLogitsProcessor(g), off at 0: when n + 1 >= g, every i with history[i : i+g-1] == history[n-g+1 : n] bans
 *     history[i+g-1] (-inf); g == 1 bans every token of the history.
 *   MinNewTokensLengthLogitsProcessor(0, m, eos): while n < m, s[eos] = -inf; nothing when eos < 0.
 * log_softmax = 1 (f32 only; beam search, where HF applies the processors to log-probabilities): the row is first replaced by
 * (s - max) - log(sum exp(s - max)), so the normaliser is that of the unprocessed logits.
 * append (optional, int64 [rows]): stored at history[r][n-1] before the history is read (the token chosen since the previous call), which
 * spares the token loop a copy launch.  n <= 1024: a larger cur is AV_ERR_ARG, and with cur_dev ldh <= 1024 is required (the kernel
 * clamps n to ldh).  One launch, one workgroup per row, O(n) work plus three passes over V with log_softmax; deterministic.  With every
 * processor off, log_softmax = 0 and no append, nothing is launched.  This is avllm_logits_process_ex with a descriptor of no tables:
 * the history and its limits are checked when a processor or append reads it (see below). */
int avllm_logits_process(void* scores, int64_t ld, int64_t rows, int32_t V, int64_t* history, int64_t ldh, const int64_t* append, int32_t cur,
                         const int32_t* cur_dev, float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_new_tokens, int64_t eos,
                         int32_t log_softmax, int32_t dtype, void* stream);
/* avllm_logits_process plus HF's SequenceBiasLogitsProcessor, NoBadWordsLogitsProcessor, SuppressTokensLogitsProcessor and
 * SuppressTokensAtBeginLogitsProcessor (generate(sequence_bias=, bad_words_ids=, suppress_tokens=, begin_suppress_tokens=)), still one launch,
 * in GenerationMixin._get_logits_processor's order: [log-softmax,] sequence bias, repetition penalty, n-gram ban, bad words, min_new_tokens,
 * suppress, begin-suppress; each reads the scores the previous one left.  The fields up to log_softmax are avllm_logits_process's arguments.
 * The tables are in device memory and may be shared by every step of a generate() call:
 *   sequence table (bias_* / bad_*): n entries; entry i is the ids tokens[i * AVLLM_LOGITS_MAX_SEQUENCE_LEN + j], j < lengths[i], 1 <=
 *     lengths[i] <= *_max_len <= AVLLM_LOGITS_MAX_SEQUENCE_LEN, n <= AVLLM_LOGITS_MAX_SEQUENCES.  An entry of length 1 always applies; a
 *     longer one when lengths[i] <= n (HF's rule; not lengths[i] - 1 <= n) and the row's last lengths[i] - 1 tokens equal its first ones.
 *   sequence bias: the entries must be ordered so that those with one last token are adjacent (the length-1 entry first, then HF's dict
 *     order); the biases of the entries that apply are summed in fp32 in table order from +0 and added to the last token's score once
 *     (f32 scores: HF's bits; bf16: one rounding).  No atomics; deterministic.
 *   bad words: an entry that applies sets its last token's score to -inf ([eos] entries are the caller's to drop, as HF's constructor does).
 *   suppress / begin_suppress: n_* distinct ids (n_* <= V) set to -inf, always / for a row with n == 0 generated tokens (HF's begin_index with
 *     inputs_embeds is 0).
 * Ids outside [0, V) are never used as an index.  The history and its 1024-token limit are needed only when repetition_penalty != 1,
 * no_repeat_ngram_size > 0, min_new_tokens > 0, append, or a table entry longer than one token is present; otherwise history may be NULL
 * and n = cur + *cur_dev is unbounded.  With every n_* zero this is avllm_logits_process exactly (the same launch, or none). */
#define AVLLM_LOGITS_MAX_SEQUENCES 4096
#define AVLLM_LOGITS_MAX_SEQUENCE_LEN 16
typedef struct avllm_logits_proc_desc {
    void* scores; int64_t ld; int64_t rows; int32_t V; int32_t dtype;
    int64_t* history; int64_t ldh; const int64_t* append; int32_t cur; const int32_t* cur_dev;
    float repetition_penalty; int32_t no_repeat_ngram_size; int32_t min_new_tokens; int64_t eos; int32_t log_softmax;
    const int32_t* bias_tokens; const int32_t* bias_lengths; const float* bias_values; int32_t n_bias; int32_t bias_max_len;
    const int32_t* bad_tokens; const int32_t* bad_lengths; int32_t n_bad; int32_t bad_max_len;
    const int32_t* suppress; int32_t n_suppress;
    const int32_t* begin_suppress; int32_t n_begin_suppress;
} avllm_logits_proc_desc;
int avllm_logits_process_ex(const avllm_logits_proc_desc* d, void* stream);
/* KV-cache row gather for beam search (the `_reorder_cache` / `Cache.reorder_cache(beam_idx)` step of GenerationMixin._beam_search):
 * dst[l, r, t, :] = src[l, parent[r], t, :] for every layer l < layers, row r < dst_rows and position t0 <= t < t1, on K and V.  The caches
 * are [layers, rows, T, dkv] contiguous (f32 or bf16, any dkv); src may have fewer rows than dst (prefix broadcast after prefill) and another
 * T.  parent: int32 [dst_rows] on the device; a row whose parent is outside [0, src_rows) is left untouched.  In place (k_src == k_dst and
 * v_src == v_dst, equal shapes) is correct for every parent map with no scratch: one workgroup owns a (tensor, layer, position, column
 * chunk) slice for all rows, stages every row's source in LDS, and writes only after a barrier; rows with parent[r] == r are skipped.
 * dst_rows <= 2048.  t0 == t1 is a no-op. */
int avllm_kv_gather_rows(const void* k_src, const void* v_src, int32_t src_rows, int64_t src_T, void* k_dst, void* v_dst, int32_t dst_rows,
                         int64_t dst_T, int32_t layers, int32_t dkv, const int32_t* parent, int32_t t0, int32_t t1, int32_t dtype, void* stream);
/* KV-cache append of the general decode path: kc[b, pos0 + t, :] = k[b * T + t, :] (and v -> vc) for t < T; k, v rows of stride ld elements
 * (slices of the fused q|k|v buffer), caches [B, Tmax, d] contiguous.  pos0 + T <= Tmax and d % 4 == 0, else AV_ERR_ARG. */
int avllm_kv_append(const void* k, const void* v, int64_t ld, void* kc, void* vc, int32_t B, int32_t T, int32_t pos0, int32_t Tmax,
                    int32_t d, int32_t dtype, void* stream);
/* out[i,:] = table[ids[i],:] ; llm.get_input_embeddings() (clip_whisper_model.py:464-487) */
int avllm_embedding(const void* table, const int64_t* ids, void* out, int64_t n, int32_t d, int32_t dtype, void* stream);
int avllm_cast(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t n, void* stream);
/* y = act(x) + r (r may be NULL; y may alias x): the activation / residual steps of DeepModalityConnector (modality_connector.py:91-108) */
int avllm_act_residual(const void* x, const void* r, void* y, int64_t n, int32_t act, int32_t dtype, void* stream);
/* nn.Dropout(p) of peft's lora.Linear (lora_dropout, clip_whisper_model.py:973-982): y = x * keep / (1-p) with the
 * counter-based mask keep(seed, row*d+col, p) (csrc/common.h av_keep); the same (seed,p) regenerates the same mask. */
int avllm_dropout(const void* x, void* y, int64_t rows, int32_t d, uint32_t seed, float p, int32_t dtype, void* stream);

/* Whisper conv stem im2col (HF:models/whisper/modeling_whisper.py:618-619).
 * conv1: mel f32 [B,80,T] -> cols [B*T, Kpad] with column c*3+kw = mel[b,c,t+kw-1] (zero padded, Kpad>=240)
 * conv2: h [B*T,d] -> cols [B*(T/2), 3d] with column kw*d+c = h[b,2t'+kw-1,c]                                */
int avllm_whisper_im2col1(const float* mel, void* cols, int32_t B, int32_t n_mels, int32_t T, int32_t Kpad,
                          int32_t dtype, void* stream);
int avllm_whisper_im2col2(const void* h, void* cols, int32_t B, int32_t T, int32_t d, int32_t dtype, void* stream);
/* CLIP patchify (HF:models/clip/modeling_clip.py:202-218): frames f32 [N,3,S,S] -> [N*(S/p)^2, Kpad>=3*p*p], column
 * c*p*p + ky*p + kx ; and the class-token rows  x[n,0,:] = class_emb + pos[0,:]                                */
int avllm_clip_patchify(const float* frames, void* cols, int32_t N, int32_t S, int32_t p, int32_t Kpad, int32_t dtype,
                        void* stream);
int avllm_clip_cls_rows(const void* class_emb, const void* pos, void* x, int32_t N, int32_t tokens, int32_t d,
                        int32_t dtype, void* stream);
/* encode()+forward() glue in one pass (clip_whisper_model.py:320-374,426-450,621-707):
 * virtual sequence X[b] = [prompt_emb[b,0:P] ; fs*a[b,t] + (1-fs)*v[b,t] (zero past each length), t<L]
 * (a or v may be NULL -> the other alone, scale 1).  out[b,0:S_out] = X (S_out==P+L), AdaptiveAvgPool1d
 * (P+L > S_out) or linear interpolation align_corners=True (P+L < S_out).                                  */
int avllm_fuse_pool(const void* a, int32_t Ta, const void* v, int32_t Tv, const void* prompt_emb, int32_t P,
                    void* out, int32_t B, int32_t L, int32_t S_out, int32_t D, float fusion_scale, int32_t dtype,
                    void* stream);
/* The adjoint of avllm_fuse_pool with respect to a and v (autograd through clip_whisper_model.py:320-374,426-450,621-707; the prompt's P
 * virtual rows receive no gradient here).  dx [B,S_out,D]; da [B,Ta,D] and / or dv [B,Tv,D] are OVERWRITTEN (either may be NULL).  Ta, Tv
 * describe the forward call: Ta == 0 or Tv == 0 means that input was absent (the other alone, scale 1); with both present da carries
 * fusion_scale and dv 1 - fusion_scale.  Rows t >= L of a longer input are written as zeros (the forward truncated them).  Gather form: every
 * output element adds the dx rows whose pooling window / interpolation stencil names it, in ascending row order, in fp32: no atomics, two
 * launches are bit-identical. */
int avllm_fuse_pool_bwd(const void* dx, void* da, int32_t Ta, void* dv, int32_t Tv, int32_t P, int32_t B, int32_t L, int32_t S_out,
                        int32_t D, float fusion_scale, int32_t dtype, void* stream);
/* Per-clip modality (modality dropout in training, a mask at inference; the reference has neither: its fusion, clip_whisper_model.py:426-450,
 * treats every clip of a call alike).  One int32 mode word per batch row; any other value is read as AVLLM_MODE_BOTH. */
enum { AVLLM_MODE_BOTH = 0, AVLLM_MODE_AUDIO = 1, AVLLM_MODE_VIDEO = 2 };
/* avllm_fuse_pool with `mode` (DEVICE int32 [B]); a and v both non-NULL, the geometry (Ta, Tv, L, P, S_out) that of the two-input call.
 * Virtual row t < L of clip b (clip_whisper_model.py:426-450, then the pooling / interpolation of :621-707 as in avllm_fuse_pool):
 *   AVLLM_MODE_BOTH   fs*a[b,t] + (1-fs)*v[b,t] (zero past each length)
 *   AVLLM_MODE_AUDIO  a[b,t], scale 1, zero for t >= Ta
 *   AVLLM_MODE_VIDEO  v[b,t], scale 1, zero for t >= Tv
 * i.e. per row what avllm_fuse_pool does for a NULL input.  The stream a row does not use is NOT READ for that row (it may hold NaN).
 * Window bounds and weights are avllm_fuse_pool's expressions: modes all 0 / all 1 / all 2 give the bits of avllm_fuse_pool(a, v) /
 * (a, NULL) / (NULL, v) at the same L. */
int avllm_fuse_pool_rows(const void* a, int32_t Ta, const void* v, int32_t Tv, const void* prompt_emb, int32_t P, const int32_t* mode,
                         void* out, int32_t B, int32_t L, int32_t S_out, int32_t D, float fusion_scale, int32_t dtype, void* stream);
/* Its adjoint, in the gather form of avllm_fuse_pool_bwd (ascending dx rows, fp32, no atomics: two launches are bit-identical).  da [B,Ta,D] and
 * dv [B,Tv,D] are both required and OVERWRITTEN: a row's used stream carries scale 1 (modes 1, 2) or fusion_scale / 1 - fusion_scale (mode 0),
 * its unused stream exact zeros; rows t >= L are zeros. */
int avllm_fuse_pool_rows_bwd(const void* dx, void* da, int32_t Ta, void* dv, int32_t Tv, int32_t P, const int32_t* mode, int32_t B, int32_t L,
                             int32_t S_out, int32_t D, float fusion_scale, int32_t dtype, void* stream);
/* Draws the modes of B clips: one launch, no host sync.  With s = (seed_dev ? *seed_dev : 0) + seed + 0x6D6F6461 (apart from the LoRA mask
 * seeds base + 0 .. base + 7*layers - 1 of the same step), u = av_pair_hash(s, b) >> 8 (24 bits; csrc/common.h),
 * ta = (uint32_t)(p_drop_audio * 2^24 + 0.5) and tv likewise (of the float arguments, evaluated in double):
 *   u < ta          -> AVLLM_MODE_VIDEO (audio dropped)
 *   u >= 2^24 - tv  -> AVLLM_MODE_AUDIO (video dropped)
 *   otherwise       -> AVLLM_MODE_BOTH
 * Both probabilities in [0, 1], sum <= 1: the ranges are disjoint and no clip loses both streams.  mode_in (nullable, DEVICE int32 [B]): a row
 * given as 1 or 2 keeps it -- a clip that has one stream only is never turned into the other; mode_out may alias it.  seed_dev given
 * (avllm_step_state.dropout_seed): the launch sits in a captured step and redraws on every replay. */
int avllm_modality_draw(const int32_t* mode_in, int32_t* mode_out, int32_t B, float p_drop_audio, float p_drop_video, uint32_t seed,
                        const uint32_t* seed_dev, void* stream);
/* clip_grad_norm_ + AdamW (trainer/clip_whisper_trainer.py:457-464,171-232) on a flat fp32 buffer, no host sync:
 * sumsq accumulates sum(g^2); the step reads it, clips with coef=min(1,max_norm/(sqrt(sumsq)+1e-6)).
 * Non-finite guard (trainer :444-452 skips backward + optimizer on a NaN/Inf loss): when *sumsq or *guard (e.g. the step's
 * loss_sum; may be NULL) is not finite the launch leaves p, m, v untouched and adds 1 to *skipped (device float, may be NULL). */
int avllm_grad_sumsq(const float* g, int64_t n, float* sumsq, void* stream);
/* The same sum in a fixed order (no float atomics): *sumsq = sum g^2, overwritten.  partials = scratch of nparts floats (<= 1024 are used).
 * Bit-reproducible, so data-parallel replicas that clip identical all-reduced gradients keep bit-identical parameters. */
int avllm_grad_sumsq_det(const float* g, int64_t n, float* partials, int32_t nparts, float* sumsq, void* stream);
int avllm_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int32_t step, const float* sumsq, float max_norm,
                     float grad_prescale, const float* guard, float* skipped, const avllm_step_state* state_dev, void* stream);
/* state_dev != NULL: lr and the bias corrections come from *state_dev (the `lr` and `step` arguments are ignored); a skipped step is
 * also counted in state_dev->skipped and takes state_dev->step back by one, so that neither the schedule nor Adam's bias corrections
 * advance on it (the reference skips optimizer.step() AND scheduler.step(), trainer/clip_whisper_trainer.py:444-452). */
/* The closing launch of a gradient-accumulation window: the same kernel with the gradient prescale read from DEVICE memory,
 * grad_prescale = 1 / *grad_div_dev (IEEE division; 0 where *grad_div_dev <= 0: a window without a scored token has a zero gradient and its
 * step is taken), used exactly where grad_prescale is used above: norm = sqrt(*sumsq) * prescale, g * prescale * clip coefficient.  The
 * guard, the skipped bookkeeping and the state_dev rule are the same; in addition state_dev->reserved[0] (avllm_step_advance_micro's count)
 * is set to 0, whether the step is taken or skipped. */
int avllm_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int32_t step, const float* sumsq, float max_norm,
                         const float* grad_div_dev, const float* guard, float* skipped, const avllm_step_state* state_dev, void* stream);
/* The same two operations over several flat buffers as ONE optimizer step (clip_grad_norm_(model.parameters()) is one global norm,
 * trainer :457-460; _setup_optimizer :183-197 gives weights `weight_decay` and biases 0): the sum of squares runs over the nbuf buffers in
 * index order with fixed-order partials (nparts >= nbuf; the <= 1024 slots are shared in proportion to the buffers' lengths), and the AdamW launch updates every segment (host array, nseg <= 8) under ONE
 * guard decision: a non-finite *sumsq / *guard leaves every segment untouched, adds 1 to *skipped and to state_dev->skipped once and takes
 * state_dev->step back once. */
int avllm_grad_sumsq_det_multi(const float* const* g, const int64_t* n, int32_t nbuf, float* partials, int32_t nparts, float* sumsq,
                               void* stream);
typedef struct avllm_adamw_seg {
    float *p, *m, *v;
    const float* g;
    int64_t n;
    float weight_decay;
    int32_t reserved;
} avllm_adamw_seg;
int avllm_adamw_step_multi(const avllm_adamw_seg* segs, int32_t nseg, float lr, float beta1, float beta2, float eps, int32_t step,
                           const float* sumsq, float max_norm, float grad_prescale, const float* guard, float* skipped,
                           const avllm_step_state* state_dev, void* stream);
/* avllm_adamw_step_multi with the device-side divisor of avllm_adamw_step_dev (same kernel, same rule). */
int avllm_adamw_step_multi_dev(const avllm_adamw_seg* segs, int32_t nseg, float lr, float beta1, float beta2, float eps, int32_t step,
                               const float* sumsq, float max_norm, const float* grad_div_dev, const float* guard, float* skipped,
                               const avllm_step_state* state_dev, void* stream);
/* build the four padded operand images of one LoRA pair from the fp32 masters A [r,din], B [dout,r]:
 * A_pad [64,din], AT_pad [din,64] (row stride ld_at), B_pad [dout,64], BT_pad [64,dout] in `dtype` */
int avllm_lora_pack(const float* A, const float* Bm, int32_t r, int32_t din, int32_t dout, void* A_pad, void* AT_pad,
                    int64_t ld_at, void* B_pad, void* BT_pad, int32_t dtype, void* stream);
/* the same for every adapter of a model in one launch: `items_dev` is a table of n rows in DEVICE memory (built once).
 * Only the r real rank rows/columns are written: the images must be zero-initialised once (their padding never changes). */
typedef struct avllm_lora_pack_item {
    const float *A, *B;              /* fp32 masters: A [r,din], B [dout,r] */
    void *A_pad, *AT_pad, *B_pad, *BT_pad;
    int64_t ld_at, dout;
} avllm_lora_pack_item;
int avllm_lora_pack_batch(const avllm_lora_pack_item* items_dev, int32_t n, int32_t r, int32_t din, int32_t dtype, void* stream);
/* fold one LoRA pair into its frozen matrix, in place (decode-time merge, once per load): W[n,k] <- round(W[n,k] + scale * sum_{j<r} B[n*r+j] *
 * A[j*K+k]).  W [N,K] in `dtype` (f32 or bf16), row stride ldw elements, 16-byte aligned, K % 8 == 0, ldw % 8 == 0; it may be a row slice of a
 * larger matrix (k_proj inside wqkv).  A [r,K], B [N,r]: the contiguous fp32 masters (not the padded images), 1 <= r <= AVLLM_LORA_PAD.
 * fp32 arithmetic: one fma chain over j ascending, one fma with scale and W, one round-to-nearest-even store; no atomics, so equal inputs give
 * equal bytes.  scale == 0 leaves W untouched. */
int avllm_lora_merge(void* W, int64_t ldw, int32_t N, int32_t K, const float* A, const float* B, int32_t r, float scale, int32_t dtype,
                     void* stream);

/* ---------------------------------------------------------------- input features on device ----------------
 * The reference builds the hot path's inputs on CPU workers, one sample at a time (src/clip_whisper/data/simple_dataset.py):
 *   audio :156-186  whisper_processor(audio, sampling_rate=16000).input_features then F.layer_norm(features, features.shape)
 *   video :191-264  clip_processor(images=frame)["pixel_values"] per RGB uint8 frame
 * These entry points do the same arithmetic on the GPU from the raw samples / raw uint8 frames (4x fewer PCIe bytes for
 * video than fp32 pixel_values).  Tables/plans are small device buffers the caller allocates and initialises once
 * (synchronous copy); the compute calls only enqueue kernels. */

/* Whisper log-mel: wave f32 [B, n] (row stride ld, mono 16 kHz, rows zero-padded to n; n > 480000 is truncated) ->
 * out f32 [B,80,3000]: 30 s zero pad, reflect pad 200, Hann(400) hop 160, |DFT|^2 (float64), slaney mel 80, log10, clamp to
 * max-8, (x+4)/4 (WhisperFeatureExtractor, feature_extraction_whisper.py:105-133); normalize != 0 adds the dataset's
 * whole-tensor layer norm (simple_dataset.py:181-183). */
size_t avllm_logmel_table_bytes(void);
int avllm_logmel_table_init(void* table_dev, int32_t n_mels);      /* n_mels: 80 (Whisper tiny..large-v2) or 128 (large-v3: feature_size=128) */
size_t avllm_logmel_workspace_bytes(int32_t B, int32_t n_mels);
int avllm_logmel(const void* table, const float* wave, int32_t B, int32_t n, int64_t ld, int32_t normalize, int32_t n_mels, float* out,
                 void* ws, size_t ws_bytes, void* stream);      /* out f32 [B, n_mels, 3000]; n_mels must be the table's */

/* CLIPImageProcessor on device: frames u8 [N,H,W,3] RGB -> out [N,3,image,image] (dtype f32 or bf16): resize so the shorter
 * edge is `image` (Pillow BICUBIC, bit-exact 8-bit fixed point: horizontal pass, uint8, vertical pass), centre crop, x/255,
 * (x-mean)/std.  A plan is specific to (H, W, image, mean, std). */
size_t avllm_clip_preproc_plan_bytes(int32_t H, int32_t W, int32_t image);
int avllm_clip_preproc_plan_init(void* plan_dev, int32_t H, int32_t W, int32_t image, const float* mean3, const float* std3);
size_t avllm_clip_preproc_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t image);
int avllm_clip_preproc(const void* plan, const uint8_t* frames, int32_t N, int32_t H, int32_t W, int32_t image, void* out,
                       int32_t dtype, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- acoustic augmentation on the device ----------------
 * No counterpart in the reference (it has no augmentation): additive noise at a target SNR on the raw waveform, in front of avllm_logmel, and
 * SpecAugment on the features it writes.  Both draw from the counter hash of csrc/common.h (av_pair_hash) with the launch seed
 * (seed_dev ? *seed_dev : 0) + seed, like avllm_modality_draw, and neither syncs with the host. */
typedef struct avllm_noise_info {
    int32_t applied;      /* 1: noise was mixed into the clip */
    int32_t row, offset;  /* the noise recording and the position in it where the segment starts (always the drawn values) */
    float snr_db;         /* the SNR asked for (given or drawn) */
    float gain;           /* the factor on the noise; 0 when applied == 0 */
} avllm_noise_info;
/* out[b] = wave[b] + gain_b * (a segment of one noise recording), the gain set so that the clip's signal-to-noise ratio is snr_b dB.
 *   wave f32 [B, n], row stride ld; len DEVICE int32 [B] | NULL (= n for every clip; values are clamped to [0, n]).
 *   noise f32 [Nn, .], row stride ld_noise; noise_len DEVICE int32 [Nn], each in [1, ld_noise] (a value outside is read as the nearest bound).
 *   snr_db DEVICE f32 [B] | NULL (then drawn from [snr_lo, snr_hi]); p_apply in [0, 1]; out f32 [B, n], row stride ld_out; out may BE wave
 *   (same pointer and stride), no other overlap; info DEVICE [B]; ws: avllm_wave_add_noise_workspace_bytes(B, n) bytes, 8-byte aligned.
 * The rule, for clip b, with s = (seed_dev ? *seed_dev : 0) + seed + 0x6E6F6973 and h_j = av_pair_hash(s, 4*b + j), j = 0..3:
 *   applied = (h_0 >> 8) < (uint32_t)(p_apply * 2^24 + 0.5) (of the float argument, evaluated in double) and len_b > 0
 *   row     = ((uint64_t)h_1 * Nn) >> 32
 *   offset  = ((uint64_t)h_2 * noise_len[row]) >> 32
 *   snr     = snr_db ? snr_db[b] : (float)((double)snr_lo + ((double)snr_hi - (double)snr_lo) * ((h_3 >> 8) * 2^-24))      (double, each
 *             operation rounded once, nothing fused)
 *   z_i     = noise[row][(offset + i) mod noise_len[row]]: the segment wraps around the end of the recording as often as it has to
 *   Es = sum_{i < len_b} w_i^2, En = sum_{i < len_b} z_i^2, in double, in a FIXED order: one partial per chunk of
 *        avllm_wave_add_noise_chunk() samples into ws, the partials folded in index order.  No atomics: a repeated launch gives the same
 *        bits.  En is the energy of the segment actually used, not of the whole recording.
 *   gain = (float)sqrt(Es / (En * pow(10, (double)snr / 10))), in double.  If Es or En is zero or not finite, or the gain is zero or not
 *          finite: gain = 0 and applied = 0.
 *   out_i = w_i + gain * z_i for i < len_b, in float32: the product rounded, then the sum rounded (no fma).
 * Positions i >= len_b of every row, and the whole row of a clip that is not mixed, are copied bit for bit (NaN payloads, -0) and never
 * enter a sum.  NO clipping and NO renormalisation: the mixture can leave [-1, 1]; the log-mel that follows has no range limit.
 * row and offset do not depend on the SNR: a sweep over SNR values at one seed mixes the same segment into each clip, only the gain changes.
 * Two launches (energies, then the mix; one when p_apply rounds to 0); 16-byte accesses on wave and out when both bases are 16-byte aligned
 * and both strides multiples of 4, a scalar form otherwise, with equal bits. */
int32_t avllm_wave_add_noise_chunk(void);
size_t avllm_wave_add_noise_workspace_bytes(int32_t B, int32_t n);
int avllm_wave_add_noise(const float* wave, int64_t ld, const int32_t* len, int32_t B, int32_t n, const float* noise, int64_t ld_noise,
                         const int32_t* noise_len, int32_t Nn, const float* snr_db, float snr_lo, float snr_hi, float p_apply, uint32_t seed,
                         const uint32_t* seed_dev, float* out, int64_t ld_out, avllm_noise_info* info, void* ws, size_t ws_bytes,
                         void* stream);
/* SpecAugment in place on feat f32 [B, M, T] (contiguous): n_time time masks, then n_freq frequency masks, n_time + n_freq <= 32.
 *   valid DEVICE int32 [B] | NULL (= T): the frames a clip really has, clamped to [0, T]; spans DEVICE int32 [B, n_time + n_freq, 2] receives
 *   (start, width) of every mask, time masks first.
 * The rule, for mask j of clip b, with s = (seed_dev ? *seed_dev : 0) + seed + 0x73706563, h = av_pair_hash(s, 64*b + 2*j) and
 * h' = av_pair_hash(s, 64*b + 2*j + 1):
 *   time mask (j < n_time):  extent = valid_b, wmax = min(max_time_width, floor(max_time_ratio * valid_b)) (the product in double)
 *   frequency mask:          extent = M,       wmax = min(max_freq_width, M); it covers all T frames, valid or not
 *   w     = ((uint64_t)h * (wmax + 1)) >> 32                  (0 .. wmax, both ends included)
 *   start = ((uint64_t)h' * (extent - w + 1)) >> 32           (start + w <= extent)
 * A cell inside any span becomes `fill`; every other cell is neither read nor written and keeps its bits.  valid_b = 0 gives zero-width time
 * spans.  One launch; with n_time + n_freq == 0 the call returns without a launch (feat and spans may then be NULL). */
int avllm_spec_augment(float* feat, int32_t B, int32_t M, int32_t T, const int32_t* valid, int32_t n_time, int32_t max_time_width,
                       float max_time_ratio, int32_t n_freq, int32_t max_freq_width, float fill, uint32_t seed, const uint32_t* seed_dev,
                       int32_t* spans, void* stream);

/* ---------------------------------------------------------------- visual augmentation on the device ----------------
 * No counterpart in the reference (it has no augmentation): the video half of the AV-HuBERT / auto-avsr recipe, folded into the two passes of
 * avllm_clip_preproc: a random crop of a slightly larger resize, a horizontal flip, and masked spans of frames.  ONE draw per clip, so the
 * mouth motion stays coherent across the frames.  The draws come from the counter hash of csrc/common.h (av_pair_hash) with the launch seed
 * (seed_dev ? *seed_dev : 0) + seed, like the acoustic augmentation, under a salt of their own; no call syncs with the host.
 *
 * The plan: specific to (H, W, resize, image, mean, std), resize >= image.  The resized shape (newH, newW) is avllm_clip_preproc's
 * shortest-edge rule applied to `resize`: short edge -> resize, long edge -> int(resize * long / short).  The plan holds Pillow's bounds and
 * coefficients of ALL newW columns and ALL newH rows (a crop window is chosen per call) and the same rescale / normalise table.  It is
 * registered at init and checked at call time. */
size_t avllm_clip_preproc_aug_plan_bytes(int32_t H, int32_t W, int32_t resize, int32_t image);      /* 0 for a shape no plan can be made for */
int avllm_clip_preproc_aug_plan_init(void* plan_dev, int32_t H, int32_t W, int32_t resize, int32_t image, const float* mean3,
                                     const float* std3);
typedef struct avllm_video_aug_info {
    int32_t left, top;    /* the crop window's corner in the resized frame (-1, -1 from avllm_video_frames_augment) */
    int32_t flip;         /* 1: the clip is mirrored left to right */
    int32_t masked;       /* the number of frames inside the union of the spans */
} avllm_video_aug_info;
/* One clip per call: frames u8 [N, H, W, 3] RGB -> out [N, 3, image, image] (dtype f32 or bf16).  clip >= 0: the clip's index in its batch
 * (the key of its draw); info DEVICE [1]; spans DEVICE int32 [n_time, 2] (may be NULL when n_time == 0); ws: at least
 * avllm_clip_preproc_aug_workspace_bytes bytes.
 * The rule, with s = (seed_dev ? *seed_dev : 0) + seed + 0x76696465 and h_j = av_pair_hash(s, 64*clip + j):
 *   left  = random_crop ? ((uint64_t)h_0 * (newW - image + 1)) >> 32 : (newW - image) / 2      (0 .. newW - image, both ends included)
 *   top   = random_crop ? ((uint64_t)h_1 * (newH - image + 1)) >> 32 : (newH - image) / 2
 *   flip  = (h_2 >> 8) < (uint32_t)(p_flip * 2^24 + 0.5)      (of the float argument, evaluated in double)
 *   time mask m < n_time <= 16:
 *     wmax  = min(max_time_width, floor(max_time_ratio * N))  (the product in double)
 *     w     = ((uint64_t)h_{4+2m} * (wmax + 1)) >> 32         (0 .. wmax, both ends included)
 *     start = ((uint64_t)h_{5+2m} * (N - w + 1)) >> 32        (start + w <= N)
 *     spans[m] = (start, w); info.masked = the number of frames n with start <= n < start + w for some m
 *   R_n = Pillow's BICUBIC resize of frame n to newH x newW: horizontal pass, uint8, vertical pass, avllm_clip_preproc's arithmetic
 *   out[n, ch, y, x] = lut[ch][ R_n[top + y][left + (flip ? image - 1 - x : x)][ch] ],  lut[ch][v] = ((float)(v / 255.0) - mean[ch]) / std[ch]
 *     i.e. crop, THEN flip: torchvision's Resize -> RandomCrop -> RandomHorizontalFlip.  One left, top and flip serve every frame of the clip.
 *   every element of a frame inside a span is `fill` converted to dtype (after the table, not before it); such a frame's pixels are not read.
 * f32 output is the table's value; bf16 output is rounded the way avllm_clip_preproc rounds.  With resize == image, random_crop = 0,
 * p_flip = 0 and n_time = 0 the output equals avllm_clip_preproc's bit for bit.  No atomics: a repeated launch repeats its bits.
 * Two launches, as avllm_clip_preproc: the horizontal pass produces only the `image` columns of the crop window (mirrored there when the clip
 * flips: the flip is an index change, not a pass) and only the input rows that the vertical taps of rows top .. top + image - 1 reach, and it
 * skips masked frames; the vertical pass writes `fill` into those.  Every workgroup recomputes the draw from (s, clip): there is no draw launch.
 * AV_ERR_ARG, naming the argument: resize < image, n_time > 16 or negative, a negative max_time_width, p_flip or max_time_ratio outside
 * [0, 1], clip < 0, a plan made for another (H, W, resize, image), a workspace that is too small. */
size_t avllm_clip_preproc_aug_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t resize, int32_t image);
int avllm_clip_preproc_aug(const void* plan, const uint8_t* frames, int32_t N, int32_t H, int32_t W, int32_t resize, int32_t image,
                           int32_t clip, int32_t random_crop, float p_flip, int32_t n_time, int32_t max_time_width, float max_time_ratio,
                           float fill, uint32_t seed, const uint32_t* seed_dev, void* out, int32_t dtype,
                           avllm_video_aug_info* info, int32_t* spans, void* ws, size_t ws_bytes, void* stream);
/* Flip and frame masks IN PLACE on pixel_values [B, F, 3, image, image] (contiguous, dtype f32 or bf16) that were resized and cropped before.
 *   nframes DEVICE int32 [B] | NULL (= F): the frames a clip really has, clamped to [0, F]; info DEVICE [B]; spans DEVICE int32 [B, n_time, 2].
 * Clip b uses the keys of clip = first_clip + b with N = nframes[b]: exactly the flip and the spans avllm_clip_preproc_aug gives that clip.
 * left and top are reported as -1.  A masked frame becomes `fill`; a frame of a flipped clip that is not masked has every row of its three
 * planes reversed (the bits are moved, nothing is computed).  Frames at or past nframes[b], and every cell that neither flips nor is masked
 * (the centre column of an odd image among them), are neither read nor written.  One launch; with p_flip rounding to 0 and n_time == 0 there
 * is none and pixels, info and spans may be NULL.  16-byte (f32) / 8-byte (bf16) accesses when image % 4 == 0 and pixels is 16-byte aligned,
 * a scalar form otherwise, with equal bits. */
int avllm_video_frames_augment(void* pixels, int32_t dtype, int32_t B, int32_t F, int32_t image, const int32_t* nframes, int32_t first_clip,
                               float p_flip, int32_t n_time, int32_t max_time_width, float max_time_ratio, float fill, uint32_t seed,
                               const uint32_t* seed_dev, avllm_video_aug_info* info, int32_t* spans, void* stream);

/* Live kernel timing for bench.py: between begin and end every avllm_gemm launch (direct or inside the model-level
 * calls) is bracketed by two HIP events on its stream.  out[0]=sum of GEMM ms, out[1]=sum of algorithmic FLOPs
 * (2*M*N*(K+K2)), out[2]=launches timed. */
int avllm_profile_begin(int32_t max_launches);
int avllm_profile_enable(int32_t on);      /* pause (0) / resume (1) bracketing between begin and end; recorded launches are kept */
int avllm_profile_end(double* out);

/* ---------------------------------------------------------------- model level ------------------ */

/* one pre-LN transformer encoder block with biases (Whisper encoder layer / CLIP encoder layer) */
typedef struct avllm_enc_layer {
    const void *ln1_w, *ln1_b;
    const void *wqkv, *bqkv;     /* [3d,d], [3d]  rows = [q;k;v]; whisper k bias = 0 */
    const void *wo, *bo;
    const void *ln2_w, *ln2_b;
    const void *w1, *b1, *w2, *b2;
    /* fp8 mode (avllm_whisper.fp8 / avllm_clip.fp8 != 0): the four weight matrices once more as block-scaled fp8 (avllm_mx_quantize layout 1):
     * codes [rows, K] and scale images.  The bf16 matrices above are then unused by the encoder forward. */
    const void *wqkv8, *sqkv8, *wo8, *so8, *w18, *s18, *w28, *s28;
} avllm_enc_layer;

typedef struct avllm_whisper {
    int32_t dtype, d, heads, layers, ffn, n_mels, n_ctx, k1pad;
    const void *conv1_w, *conv1_b;   /* [d,k1pad] (col c*3+kw, zero padded), [d] */
    const void *conv2_w, *conv2_b;   /* [d,3d] (col kw*d+c), [d] */
    const void* pos;                 /* [n_ctx,d] */
    const avllm_enc_layer* layer;    /* host array [layers] */
    const void *lnf_w, *lnf_b;
    int32_t fp8;                     /* 1: layer projections run on the block-scaled fp8 matrix pipe (dtype must be AVLLM_BF16) */
} avllm_whisper;
size_t avllm_whisper_workspace_bytes(const avllm_whisper* w, int32_t B);
/* ClipWhisperModel.encode_audio minus the connector (clip_whisper_model.py:1067-1104 ->
 * WhisperEncoder.forward): mel f32 [B,80,2*n_ctx] -> out [B,n_ctx,d] */
int avllm_whisper_encoder_fwd(const avllm_whisper* w, const float* mel, int32_t B, void* out, void* ws,
                              size_t ws_bytes, void* stream);

typedef struct avllm_clip {
    int32_t dtype, d, heads, layers, ffn, image, patch, tokens;
    float eps;
    const void* patch_w;             /* [d, 3*p*p] */
    const void *class_emb, *pos;     /* [d], [tokens,d] */
    const void *pre_ln_w, *pre_ln_b;
    const avllm_enc_layer* layer;    /* host array [layers] */
    int32_t fp8;                     /* as avllm_whisper.fp8 */
    int32_t frames_bf16;             /* 1: `frames` of avllm_clip_vision_cls_fwd are bf16 (what avllm_clip_preproc writes with dtype bf16: half the bytes
                                      * of the reference's fp32 pixel_values on the way into the patch embedding) */
} avllm_clip;
size_t avllm_clip_workspace_bytes(const avllm_clip* c, int32_t N);
/* ClipWhisperModel.encode_video minus the connector (clip_whisper_model.py:1108-1142 -> CLIPVisionModel.forward,
 * last_hidden_state[:,0], no post_layernorm): frames f32 [N,3,S,S] -> cls [N,d] */
int avllm_clip_vision_cls_fwd(const avllm_clip* c, const void* frames, int32_t N, void* cls, void* ws,
                              size_t ws_bytes, void* stream);

typedef struct avllm_lora_mod {      /* padded operand images (see avllm_lora_pack); NULL = no adapter */
    const void *A_pad, *AT_pad, *B_pad, *BT_pad;
    int64_t ld_at;                   /* row stride of AT_pad: 64, or 192 when q/k/v share one [din,192] image */
    float *gA, *gB;                  /* fp32 grads [r,din], [dout,r] (accumulated) */
} avllm_lora_mod;

typedef struct avllm_llama_layer {
    const void *ln1_w, *ln2_w;
    const void *wqkv;                /* [d+2*dkv, d] rows [q;k;v]  (dkv = kv_heads*hd; 3d without GQA) */
    const void *wo;                  /* [d,d] */
    const void *wgu;                 /* [2f,d] rows [gate;up] */
    const void *wdown;               /* [d,f] */
    /* transposed images for dX = dY.W (training only; NULL for inference): */
    const void *wqkv_t;              /* [d, d+2*dkv] */
    const void *wo_t;                /* [d,d] */
    const void *wgu_t;               /* [d,2f] */
    const void *wdown_t;             /* [f,d] */
    avllm_lora_mod lora[4];          /* q,k,v,o */
    /* fp8 mode (avllm_llama.fp8 != 0): forward-pass images of the four frozen matrices (avllm_mx_quantize layout 1).  The backward pass keeps
     * using the bf16 transposed images: gradients are not quantised. */
    const void *wqkv8, *sqkv8, *wo8, *so8, *wgu8, *sgu8, *wdown8, *sdown8;
    /* fp8 token step (avllm_llama.decode_fp8 != 0): the exponent matrices [rows, K/32] (avllm_mx_quantize layout 2) of the codes wqkv8, wo8,
     * wgu8, wdown8 above, which the token step then streams instead of the bf16 matrices.  Unused otherwise. */
    const void *eqkv8, *eo8, *egu8, *edown8;
    /* fp4 token step (avllm_llama.decode_fp4 != 0): MXFP4 codes [rows, K/2] and exponent matrices [rows, K/32] of the four frozen matrices
     * (avllm_mx4_quantize).  The exponents are not those of the fp8 codes: emax differs. */
    const void *wqkv4, *wo4, *wgu4, *wdown4;
    const void *eqkv4, *eo4, *egu4, *edown4;
    /* frozen attention projection biases in the model dtype, NULL = none: bqkv [d+2*dkv] = [q;k;v] (Qwen2 / Qwen2.5, or a Llama checkpoint
     * saved with attention_bias), bo [d] (attention_bias only).  Added to the fp32 accumulator of the base product before its one rounding, on
     * every path (training forward in bf16 / fp32 / fp8, prefill, token step in every weight form); peft's order: base_layer(x) with its bias,
     * plus the adapter term, then RoPE.  No gradient is formed for them. */
    const void *bqkv, *bo;
    /* per-head RMSNorm weights of q and k, [hd] each in the model dtype (Qwen3: transformers/models/qwen3/modeling_qwen3.py
     * Qwen3Attention.forward, q_norm / k_norm); NULL = none, either both or neither.  eps is the model's.  Order on every path: base_layer(x)
     * with its bias, plus the adapter term, then the head norm, then RoPE.  Frozen: no gradient is formed for them.  Qwen3-1.7B / 8B / 14B
     * geometry (hd = d / heads = 128); hd is 64 or 128. */
    const void *q_norm_w, *k_norm_w;
    /* adapters on the MLP projections: gate_proj, up_proj, down_proj (peft target_modules beyond the four attention modules, up to
     * "all-linear"); A_pad == NULL = none, any subset.  gate, up: A [r, d], B [ffn, r], input the post-attention RMSNorm output; down: A [r, ffn],
     * B [d, r], input silu(gate) * up.  Images as for lora[] (avllm_lora_pack with din = the module's input width); gate and up may share
     * one [d, 128] AT image (ld_at 128, up's at column 64) as q, k, v share one of 192 columns.  Honoured by avllm_llama_lora_fwd_loss / _bwd,
     * avllm_llama_prefill and the general token step; while any is attached the fused token step is not taken (avllm_llama_decode_is_fused
     * returns 0) and avllm_llama.fp8 is refused.  Appended last: no earlier offset moves. */
    avllm_lora_mod lora_mlp[3];      /* gate, up, down */
} avllm_llama_layer;

typedef struct avllm_llama {
    int32_t dtype, d, heads, layers, ffn, vocab, lora_r;
    int32_t kv_heads;                /* grouped-query attention: key/value heads (0 = heads).  wqkv is [(heads+2*kv_heads)*hd, d],
                                      * the k/v adapters' B is [kv_heads*hd, r], the KV cache rows are kv_heads*hd wide */
    float eps, theta, lora_scale;
    float lora_dropout;              /* applied by avllm_llama_lora_fwd_loss/_bwd only (training); 0 = off */
    uint32_t dropout_seed;           /* attention module j (q, k, v, o) of layer l uses seed dropout_seed + 4*l + j; MLP module k (0 gate, 1 up,
                                      * 2 down) of layer l uses dropout_seed + 4*layers + 3*l + k.  The mask index of an element is row * K + col
                                      * with K the module's input width (d; ffn for down): what avllm_dropout gives on [M, K].  Change it
                                      * every step */
    const uint32_t* dropout_seed_dev;/* optional DEVICE word added to dropout_seed at run time (graph-replayable steps: avllm_step_state) */
    const void* embed;               /* [vocab,d] */
    const void* norm_w;
    const void* lm_head;             /* [vocab,d] */
    const void* lm_head_t;           /* [d,vocab] (training) */
    const avllm_llama_layer* layer;  /* host array [layers] */
    int32_t fp8;                     /* 1: the frozen projections of avllm_llama_lora_fwd_loss (q/k/v/o base terms, gate/up, down, lm_head) run on
                                      * the block-scaled fp8 matrix pipe (BASELINE config 5); LoRA terms, attention, norms and the whole
                                      * backward pass stay bf16 */
    const void *lm_head8, *slm_head8;
    /* rope_orig_ctx > 0: "llama3" RoPE frequency scaling of Llama-3.1 / 3.2 checkpoints (config.json rope_scaling: factor, low_freq_factor,
     * high_freq_factor, original_max_position_embeddings; HF:modeling_rope_utils.py _compute_llama3_parameters).  0 = plain RoPE. */
    float rope_factor, rope_low_freq_factor, rope_high_freq_factor;
    int32_t rope_orig_ctx;
    /* 1: weight-only fp8 token step.  When the fused path applies (avllm_llama_decode_is_fused: B <= 16), the q|k|v, o, gate|up, down
     * projections and lm_head of avllm_llama_decode_step(_at) stream the e4m3 codes (wqkv8 .. wdown8, lm_head8) with the layout-2 exponents
     * (eqkv8 .. edown8, elm_head8) instead of the bf16 matrices; activations, KV cache, attention, norms, adapters and logits are unchanged.
     * Needs bf16, d, ffn multiples of 128 and vocab a multiple of 16.  B > 16 and prefill stay on the bf16 matrices.  Independent of fp8. */
    int32_t decode_fp8;
    const void* elm_head8;
    /* 1: weight-only fp4 token step.  As decode_fp8, but the q|k|v, o, gate|up and down projections of the fused step (B <= 16) stream the
     * MXFP4 codes (wqkv4 .. wdown4, eqkv4 .. edown4); lm_head -- 2 % of the bytes, and the matrix whose rounding moves the argmax most --
     * streams as e4m3 (lm_head8, elm_head8).  Same shape conditions as decode_fp8; not together with it. */
    int32_t decode_fp4;
    /* 1: the KV cache handed to avllm_llama_prefill / avllm_llama_decode_step(_at) is the block-scaled e4m3 image (csrc/kv_fp8.hip): for K and
     * for V the codes uint8 [layers, B, Tmax, dkv] followed by the E8M0 exponents uint8 [layers, B, Tmax, dkv/32], one per 32 consecutive
     * elements of a row, by avllm_mx_quantize's rule (avllm_llama_kv_cache_bytes each, 33/64 of the bf16 bytes; base 16-byte aligned).  K is
     * stored after RoPE (and the head norm), V as projected; a token attends to its own row as stored.  The prefill's own attention is
     * unchanged (only its append quantises); the token step must be the fused one (avllm_llama_decode_caches_fp8), else AV_ERR_ARG.  Needs
     * bf16 and a head dim of 64 or 128.  0: the cache is [layers][B][Tmax][dkv] in the model dtype, as ever. */
    int32_t kv_fp8;
} avllm_llama;

size_t avllm_llama_train_workspace_bytes(const avllm_llama* m, int32_t B, int32_t S);
/* self.llm(inputs_embeds, attention_mask=ones, labels) (clip_whisper_model.py:602-613 ->
 * LlamaForCausalLM.forward HF:models/llama/modeling_llama.py:435-488 + ForCausalLMLoss).
 * x [B,S,d]; labels int64 [B,S] with -100 already applied; logits [B,S,vocab] written when non-NULL
 * (always materialised internally in this version).  loss_sum/count accumulate (zero first); activations for
 * the backward pass stay in `ws`. */
int avllm_llama_lora_fwd_loss(const avllm_llama* m, const void* x, const int64_t* labels, int32_t B, int32_t S,
                              void* logits, float* loss_sum, float* count, void* ws, size_t ws_bytes, void* stream);
/* loss.backward() for the LoRA tensors only (frozen base weights => dX GEMMs + LoRA dA/dB).
 * Must follow avllm_llama_lora_fwd_loss with the same ws.  Gradient of  grad_scale * loss_sum / *count.
 * `after_layer` (may be NULL) is called on the host right after layer i's kernels are enqueued (31 -> 0) so a
 * data-parallel caller can launch that layer's gradient all-reduce on a side stream. */
typedef void (*avllm_layer_cb)(int32_t layer, void* user);
int avllm_llama_lora_bwd(const avllm_llama* m, const int64_t* labels, int32_t B, int32_t S, const float* count,
                         float grad_scale, void* ws, size_t ws_bytes, avllm_layer_cb after_layer, void* user,
                         void* stream);
/* The same backward pass in pieces: decoder layers layer_hi, layer_hi-1, ..., layer_lo (inclusive).  The piece that starts at the
 * last layer (layer_hi == layers-1) also runs the loss / lm_head / final-norm part; consecutive pieces must be called in descending
 * order on the same ws (the running residual gradient stays there).  Lets a data-parallel caller replay each piece from its own
 * hipGraph and launch that piece's gradient all-reduce while the next piece runs. */
int avllm_llama_lora_bwd_layers(const avllm_llama* m, const int64_t* labels, int32_t B, int32_t S, const float* count,
                                float grad_scale, void* ws, size_t ws_bytes, int32_t layer_hi, int32_t layer_lo,
                                avllm_layer_cb after_layer, void* user, void* stream);
/* The same with the gradient of the loss with respect to inputs_embeds (what the connectors need when they train: with
 * freeze_encoders=False the reference's autograd carries it on through encode(), clip_whisper_model.py:1096-1106,1136-1146).  dx_embeds
 * [B*S, d] in the engine dtype, may be NULL (= the call above).  When it is given and the piece reaches layer_lo == 0, layer 0 also runs
 * the dqkv . Wqkv product with the adapters' input gradient and the input-RMSNorm backward that layers > 0 run, and d resid[0] is left in
 * dx_embeds.  The workspace layout is unchanged. */
int avllm_llama_lora_bwd_layers_dx(const avllm_llama* m, const int64_t* labels, int32_t B, int32_t S, const float* count,
                                   float grad_scale, void* ws, size_t ws_bytes, int32_t layer_hi, int32_t layer_lo,
                                   avllm_layer_cb after_layer, void* user, void* dx_embeds, void* stream);
/* The training objective with label smoothing and the z-loss (avllm_ce_smooth_fwd's rule): label_smoothing in [0, 1), z_loss >= 0, else
 * AV_ERR_ARG.  loss_terms: optional device memory [3]; with either value non-zero the forward adds the raw sums of nll, u and q onto it (zero
 * it first).  The two entries below are avllm_llama_lora_fwd_loss and avllm_llama_lora_bwd_layers_dx with that objective: the backward takes
 * the options its forward took.  opts == NULL, or both values 0: exactly the launches of the entries without options (the plain cross
 * entropy; loss_terms is left alone).  The options are an argument, not fields of avllm_llama: the descriptor keeps its layout. */
typedef struct {
    float label_smoothing, z_loss;
    float* loss_terms;
} avllm_loss_opts;
int avllm_llama_lora_fwd_loss_opts(const avllm_llama* m, const void* x, const int64_t* labels, int32_t B, int32_t S, void* logits,
                                   float* loss_sum, float* count, const avllm_loss_opts* opts, void* ws, size_t ws_bytes, void* stream);
int avllm_llama_lora_bwd_layers_dx_opts(const avllm_llama* m, const int64_t* labels, int32_t B, int32_t S, const float* count,
                                        float grad_scale, void* ws, size_t ws_bytes, int32_t layer_hi, int32_t layer_lo,
                                        avllm_layer_cb after_layer, void* user, void* dx_embeds, const avllm_loss_opts* opts, void* stream);

/* Inference: prefill on inputs_embeds and single-token steps with a KV cache (llm.generate,
 * clip_whisper_model.py:1337-1340 -> GenerationMixin greedy).  kcache/vcache [layers][B][Tmax][d].
 * prefill writes positions [0,S) and returns the hidden state of the LAST position after the final norm
 * -> logits_last [B,vocab] f32; decode_step embeds `ids` [B], runs position `pos`, returns logits [B,vocab]. */
size_t avllm_llama_infer_workspace_bytes(const avllm_llama* m, int32_t B, int32_t S);
int avllm_llama_prefill(const avllm_llama* m, const void* x, int32_t B, int32_t S, void* kcache, void* vcache,
                        int32_t Tmax, float* logits_last, void* all_logits, void* ws, size_t ws_bytes, void* stream);
int avllm_llama_decode_step(const avllm_llama* m, const int64_t* ids, int32_t B, int32_t pos, void* kcache,
                            void* vcache, int32_t Tmax, float* logits, void* ws, size_t ws_bytes, void* stream);
/* The same step with the position in DEVICE memory: the token runs at position pos + *pos_dev (pos_dev may be NULL), so a captured
 * hipGraph of the step can be replayed for every token (advance *pos_dev between replays, e.g. with avllm_step_advance's sibling
 * avllm_pos_advance).  The caller guarantees pos + *pos_dev < Tmax. */
int avllm_llama_decode_step_at(const avllm_llama* m, const int64_t* ids, int32_t B, int32_t pos, const int32_t* pos_dev, void* kcache,
                               void* vcache, int32_t Tmax, float* logits, void* ws, size_t ws_bytes, void* stream);
/* 1 when a token step of B sequences on this model takes the fused bf16 path (one launch per projection + one attention launch per
 * layer), 0 when it takes the general path: tests and benchmarks assert which one they measured. */
int avllm_llama_decode_is_fused(const avllm_llama* m, int32_t B);
/* 1 when a token step of B sequences streams the fp8 weight images (decode_fp8 set and the fused path taken), 0 when it reads bf16. */
int avllm_llama_decode_streams_fp8(const avllm_llama* m, int32_t B);
/* The same for the fp4 weight images (decode_fp4).  A decode_fp4 model answers 0 to the fp8 query. */
int avllm_llama_decode_streams_fp4(const avllm_llama* m, int32_t B);
/* 1 when a token step of B sequences reads and writes the fp8 cache image (kv_fp8 set and the fused path taken), 0 otherwise: the caller
 * decides the cache's form with it when it allocates (more rows, or the fused path switched off: kv_fp8 = 0 and the bf16 cache). */
int avllm_llama_decode_caches_fp8(const avllm_llama* m, int32_t B);
/* The token step of R = B * group rows whose `group` rows per item (beams, or sampled sequences) share the item's prefix.  k_prefix / v_prefix
 * [layers][B][S][dkv] is the cache avllm_llama_prefill wrote for the B items (Tmax = S), read only; k_suffix / v_suffix [layers][R][N][dkv] hold
 * each row's own generated positions.  The token of row r runs at position S + pos (+ *pos_dev), its K/V go to suffix row pos (+ *pos_dev; a
 * device-side row outside [0, N) writes nothing), and it attends prefix rows [0, S) of item r / group followed by suffix rows [0, pos] of row
 * r (the device-side length is clamped to N).  Fused path only (avllm_llama_decode_shares_prefix), else AV_ERR_ARG; caches in the model's form
 * (kv_fp8: both are images).  Only the attention launch differs from avllm_llama_decode_step_at (avllm_attention_decode_shared).
 * ws: avllm_llama_decode_shared_workspace_bytes(m, R) bytes. */
size_t avllm_llama_decode_shared_workspace_bytes(const avllm_llama* m, int32_t R);
int avllm_llama_decode_step_shared(const avllm_llama* m, const int64_t* ids, int32_t R, int32_t group, int32_t pos, const int32_t* pos_dev,
                                   const void* k_prefix, const void* v_prefix, int32_t S, void* k_suffix, void* v_suffix, int32_t N, float* logits,
                                   void* ws, size_t ws_bytes, void* stream);
/* 1 when a token step of R rows can share prefixes: exactly where avllm_llama_decode_is_fused(m, R) is 1. */
int avllm_llama_decode_shares_prefix(const avllm_llama* m, int32_t R);
/* Bytes of ONE of the two caches (K or V) of B sequences and Tmax positions in the model's form: layers * B * Tmax * dkv elements of the model
 * dtype, or with kv_fp8 that many code bytes plus one exponent byte per 32. */
size_t avllm_llama_kv_cache_bytes(const avllm_llama* m, int32_t B, int32_t Tmax);

/* The kernels of the fp8 KV cache (csrc/kv_fp8.hip).  An image of cache rows [..., dkv] is two planes, codes uint8 [..., dkv] (e4m3fn) and
 * exponents uint8 [..., dkv/32] (E8M0, biased by 127), bit-identical to avllm_mx_quantize(layout 2) of the bf16 rows; k_codes / k_exps / v_codes /
 * v_exps below are the planes of ONE layer, [B, Tmax, dkv] and [B, Tmax, dkv/32].  bf16 only; code planes 16-byte aligned.
 * avllm_kv8_append: avllm_kv_append's fp8 twin (the prefill's append): rows k, v [B * T, dkv] of stride ld -> positions [pos0, pos0 + T).
 * pos0 + T <= Tmax, dkv % 32 == 0, ld % 8 == 0, else AV_ERR_ARG. */
int avllm_kv8_append(const void* k, const void* v, int64_t ld, void* k_codes, void* k_exps, void* v_codes, void* v_exps, int32_t B, int32_t T,
                     int32_t pos0, int32_t Tmax, int32_t dkv, void* stream);
/* The token step's append, after a raw_qkv projection: qkv [B, ld] = q [heads hd] | k [kv_heads hd] | v.  rotate = 1: q is rotated in place
 * (fp32 arithmetic on rope [hd/2][2] = cos, sin; one rounding to bf16), k is rotated in fp32 and quantised from there, v is quantised; rotate = 0
 * (a head-norm launch has rotated q and k in place already): k and v are quantised as they are, q is not touched.  The row goes to position
 * pos + *pos_dev (pos_dev may be NULL); a device-side position outside [0, Tmax) writes nothing.  hd 64 or 128. */
int avllm_kv8_rope_append(void* qkv, int64_t ld, int32_t B, int32_t heads, int32_t kv_heads, int32_t hd, const float* rope, int32_t rotate,
                          void* k_codes, void* k_exps, void* v_codes, void* v_exps, int32_t Tmax, int32_t pos, const int32_t* pos_dev, void* stream);
/* avllm_attention_decode (bf16) over the image: Tk + *tk_dev rows (clamped to Tmax), dequantised exactly in registers (code x 2^e); scores,
 * online softmax and the weighted sum in fp32.  Nothing but the cache is read for K and V. */
int avllm_attention_decode_kv8(const void* q, int64_t ldq, const void* k_codes, const void* k_exps, const void* v_codes, const void* v_exps, void* o,
                               int64_t ldo, int32_t B, int32_t H, int32_t hd, int32_t Tk, const int32_t* tk_dev, int32_t Tmax, float scale,
                               int32_t kv_group, void* stream);
/* Single-token attention over a shared prefix (csrc/attention_decode_shared.hip; bf16 q and o [R, H hd]).  Row r of R = B * group attends rows
 * [0, S) of item r / group in the prefix cache [B, Tprefix, dkv], followed by rows [0, Tk + *tk_dev) (clamped to N) of its own row of the suffix
 * cache [R, N, dkv]: the softmax over the concatenation, fp32 throughout, no atomics (identical inputs give identical bits, in every group
 * slot).  Two launches: prefix partials per (row, head, slice) into ws, then suffix + merge.  hd 64 or 128; R % group == 0; 0 < S <= Tprefix;
 * ws of avllm_attention_decode_shared_workspace_bytes(R, H, hd) bytes.  _kv8: both caches are fp8 images (planes as above), dequantised as
 * avllm_attention_decode_kv8 does. */
size_t avllm_attention_decode_shared_workspace_bytes(int32_t R, int32_t H, int32_t hd);
int avllm_attention_decode_shared(const void* q, int64_t ldq, const void* k_prefix, const void* v_prefix, int32_t S, int32_t Tprefix,
                                  const void* k_suffix, const void* v_suffix, int32_t Tk, const int32_t* tk_dev, int32_t N, void* o, int64_t ldo,
                                  int32_t R, int32_t group, int32_t H, int32_t hd, float scale, int32_t kv_group, void* ws, size_t ws_bytes,
                                  void* stream);
int avllm_attention_decode_shared_kv8(const void* q, int64_t ldq, const void* kp_codes, const void* kp_exps, const void* vp_codes, const void* vp_exps,
                                      int32_t S, int32_t Tprefix, const void* ks_codes, const void* ks_exps, const void* vs_codes, const void* vs_exps,
                                      int32_t Tk, const int32_t* tk_dev, int32_t N, void* o, int64_t ldo, int32_t R, int32_t group, int32_t H,
                                      int32_t hd, float scale, int32_t kv_group, void* ws, size_t ws_bytes, void* stream);
/* avllm_kv_gather_rows on whole fp8 images (all layers: k_src .. v_dst are the bases of [layers, rows, T, dkv] images): codes and exponents of
 * positions [t0, t1) move together, two launches of the same kernel on rows of dkv and of dkv/32 bytes.  dkv % 64 == 0. */
int avllm_kv8_gather_rows(const void* k_src, const void* v_src, int32_t src_rows, int64_t src_T, void* k_dst, void* v_dst, int32_t dst_rows,
                          int64_t dst_T, int32_t layers, int32_t dkv, const int32_t* parent, int32_t t0, int32_t t1, void* stream);
int avllm_pos_advance(int32_t* pos_dev, int32_t by, void* stream);

/* One projection of a decode token step (bf16, 1 <= M <= 16 rows, K % 128 == 0): C = epilogue(rmsnorm?(A) . W^T).  Every weight row
 * is streamed from HBM once; the fused forms remove the launches between the projections of LlamaDecoderLayer.forward:
 *   mode 0  plain: C[M,N] (+ R), bf16 or f32 out                                    (o_proj / down_proj + residual, lm_head)
 *   mode 1  SwiGLU: W = [gate; up] rows [2N, K]; C[M,N] = silu(A.gate^T) * (A.up^T)  (LlamaMLP.forward's act_fn(gate) * up)
 *   mode 2  q|k|v: W rows [dq + 2 dkv, K]; rotary embedding on q and k (pairs (i, i + hd/2), table rope[hd/2][2] = cos,sin of the
 *           position); q -> C[M,dq]; k, v -> cache rows kc/vc[m][pos + *pos_dev][dkv]  (apply_rotary_pos_emb + DynamicCache.update).
 *           hd must be a power of two >= 32 (32, 64, 128, 256, ...): any other head dim is an argument error.
 * norm_w != NULL folds the preceding RMSNorm in: x * rsqrt(mean(x^2) + eps) * norm_w is applied to A on the fly. */
typedef struct avllm_dec_proj_desc {
    const void* A; int64_t lda;
    const void* W; int64_t ldw;
    const void* norm_w; float eps;
    int32_t M, K, N, mode;
    void* C; int64_t ldc; int32_t out_f32;
    const void* R; int64_t ldr;
    int32_t dq, dkv, hd;
    const float* rope;
    void *kc, *vc;
    int32_t Tmax, pos;
    const int32_t* pos_dev;
    /* LoRA side term of peft lora.Linear, + lora_scale * B (A x), added in the epilogue (before RoPE): lora_t [M, ld_lora_t] f32 holds the
     * rank-side products of this projection's (normalised) input, module j in columns [64 j, 64 j + lora_r) -- itself a mode-0 launch over
     * the A images; lora_b[j] = padded B image [rows of module j, 64] (avllm_lora_pack).  mode 2: j = q, k, v; mode 0: j = 0; not with mode 1.
     * lora_t == NULL: no adapters. */
    const float* lora_t; int64_t ld_lora_t;
    const void* lora_b[3];
    int32_t lora_r; float lora_scale;
    /* fp8 weight form: W8 != NULL streams the weight rows as e4m3 codes [rows, K] (row stride ldw BYTES, ldw % 16 == 0, 16-byte aligned) with
     * E8 = their E8M0 exponents [rows, K/32] uint8, row-major, biased by 127 (avllm_mx_quantize layout 2); W is then ignored.  Every mode,
     * the norm fold, residual, outputs and adapters as above: the product is the bf16 form's on the weights codes * 2^(E8 - 127) (exact in
     * bf16), summed in a different fp32 order inside each 64-column pair of K-steps. */
    const void* W8; const void* E8;
    /* fp4 weight form: W4 != NULL streams the weight rows as OCP MXFP4 codes (e2m1, two per byte: element 2i of a row in the LOW nibble of
     * byte i, element 2i+1 in the high nibble; bit 3 of a code is the sign) [rows, K/2] (row stride ldw BYTES, ldw % 16 == 0, 16-byte
     * aligned) with E8 = their E8M0 exponents [rows, K/32] uint8, row-major, biased by 127 (avllm_mx4_quantize); W is then ignored.  Not
     * together with W8.  Every mode, the norm fold, residual, outputs and adapters as above: the product is the bf16 form's on the weights
     * code value * 2^(E8 - 127) (exact in bf16), summed in a different fp32 order inside each 128-column group of K-steps. */
    const void* W4;
    /* bias != NULL: bf16 [N] in the logical output column order of W's rows (mode 2: [q;k;v], not the kernel's rotary pairing), added to the
     * fp32 sum after the norm fold's scale and before the adapter term, the residual and RoPE.  Modes 0 and 2; refused in mode 1.  NULL: the
     * launch is the bias-free kernel (the epilogue is templated on the bias). */
    const void* bias;
    /* raw_qkv != 0 (mode 2 only): the projection of a model whose q and k heads are normalised before the rotary embedding (Qwen3).  A head's
     * columns belong to several workgroups, so the norm cannot sit in this epilogue: no rotation and no cache write here; q, k and v all go
     * to C[M, N] in logical column order (ldc >= N; the plain col = 16 b + fr row mapping), bias and adapter terms added exactly as above;
     * rope, kc, vc, Tmax, pos, pos_dev are ignored.  One avllm_qk_norm_rope launch in its cache form follows.  Run-time data of the same
     * kernels: with raw_qkv == 0 a launch is what it always was. */
    int32_t raw_qkv;
} avllm_dec_proj_desc;
int avllm_dec_proj(const avllm_dec_proj_desc* d, void* stream);
/* Per-head RMSNorm of q and k fused with the rotary embedding (transformers/models/qwen3/modeling_qwen3.py Qwen3Attention.forward:
 * q_norm(q_proj(x).view(.., hd)), k_norm(..), then apply_rotary_pos_emb).  x [rows, ld] is a q|k|v buffer whose first (heads + kv_heads) * hd
 * columns are the adjacent q and k slices; they are rewritten in place, v and any padding columns are never written.  For each (row, head):
 * y = x * rsqrt(mean(x^2) + eps) * w with w = q_norm_w or k_norm_w [hd] by head index (no "+1" offset), then the rotary pair (i, i + hd/2)
 * from tab [T][hd/2][2] (avllm_rope_table; row r reads table row r % T).  fp32 arithmetic, one rounding.  hd is 64 or 128; dtype f32 / bf16;
 * rows of ld elements are multiples of 16 bytes.
 *   pre, rstd (optional, training): the pre-norm q|k values [rows, (heads + kv_heads) * hd] and rstd [rows, heads + kv_heads] f32.
 *   kc, vc (optional, both or neither: the token step): T == 1 and row m is sequence m; the rotated k and the untouched v of the row go to
 *   cache row kc / vc [m][pos + *pos_dev][kv_heads * hd] (pos_dev may be NULL) when 0 <= pos + *pos_dev < Tmax and nowhere otherwise; q is
 *   rewritten in x, the k and v columns of x stay as they are. */
int avllm_qk_norm_rope(void* x, int64_t ld, int64_t rows, int32_t T, int32_t heads, int32_t kv_heads, int32_t hd, const void* q_norm_w,
                       const void* k_norm_w, float eps, const float* tab, void* pre, float* rstd, void* kc, void* vc, int32_t Tmax, int32_t pos,
                       const int32_t* pos_dev, int32_t dtype, void* stream);
/* Its backward, in place on the q and k slices of dy [rows, ld]: dy arrives as the gradient with respect to the normed PRE-RoPE heads (what
 * avllm_attention_bwd_rope leaves, or avllm_attention_bwd followed by avllm_rope_tab(inverse = 1)) and leaves as
 * dx = rstd * (g - xhat * mean(g * xhat)) with g = w * dy, xhat = pre * rstd, from the forward's saves.  No weight gradient: the norms are frozen. */
int avllm_qk_norm_bwd(void* dy, int64_t ld, int64_t rows, int32_t heads, int32_t kv_heads, int32_t hd, const void* q_norm_w, const void* k_norm_w,
                      const void* pre, const float* rstd, int32_t dtype, void* stream);
/* Single-query attention over the cache rows [0, Tk + *tk_dev) (tk_dev may be NULL) of kc/vc [B][Tmax][(H/kv_group)*hd]: one pass with
 * an online softmax; q [B, H*hd] (row stride ldq), o [B, H*hd] (ldo).  LlamaAttention.forward with q_len == 1 (eager softmax(QK^T/sqrt(hd))V). */
int avllm_attention_decode(const void* q, int64_t ldq, const void* kc, const void* vc, void* o, int64_t ldo, int32_t B, int32_t H, int32_t hd,
                           int32_t Tk, const int32_t* tk_dev, int32_t Tmax, float scale, int32_t kv_group, int32_t dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
