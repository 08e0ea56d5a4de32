// Per-clip modality: the fusion + pooling glue of elementwise.hip with one mode word per batch row (include/avllm.h, AVLLM_MODE_*), its adjoint,
// and the draw of the mode words (modality dropout).  The default path does not come here: avllm_fuse_pool / avllm_fuse_pool_bwd are untouched.
#include "common.h"
#include "avllm_internal.h"

// ---------------------------------------------------------------- forward
constexpr int FWD_VEC = 4;      // see fuse_pool_rows_kernel
// A row's mode selects which inputs exist FOR THAT ROW: mode 1 hides v, mode 2 hides a, and the virtual row is then what fuse_pool_kernel's
// virt_row computes for a NULL input (the other alone, scale 1).  The hidden input is never dereferenced.  virt_row's text, 4 wide like it (see below).
template <typename T>
__device__ __forceinline__ void virt_row_n(const T* a, int Ta, const T* v, int Tv, const T* pe, int P, int b, int j, int c, int D, float fs,
                                           float (&o)[FWD_VEC]) {
#pragma unroll
    for (int k = 0; k < FWD_VEC; ++k) o[k] = 0.f;
    if (j < P) { load_f<FWD_VEC>(pe + ((long)b * P + j) * D + c, o); return; }
    const int t = j - P;
    if (a && v) {
        float tv[FWD_VEC];
        if (t < Ta) { load_f<FWD_VEC>(a + ((long)b * Ta + t) * D + c, tv);
#pragma unroll
            for (int k = 0; k < FWD_VEC; ++k) o[k] = fs * tv[k]; }
        if (t < Tv) { load_f<FWD_VEC>(v + ((long)b * Tv + t) * D + c, tv);
#pragma unroll
            for (int k = 0; k < FWD_VEC; ++k) o[k] += (1.0f - fs) * tv[k]; }
    } else if (a) { if (t < Ta) load_f<FWD_VEC>(a + ((long)b * Ta + t) * D + c, o); }
    else { if (t < Tv) load_f<FWD_VEC>(v + ((long)b * Tv + t) * D + c, o); }
}

// grid (S_out, B): the mode is uniform per block and read once.  Window bounds and weights are fuse_pool_kernel's own expressions, so a launch of
// all-equal modes gives the bits of avllm_fuse_pool with the matching inputs.
// 4 elements per thread in both dtypes, as fuse_pool_kernel, and NOT the adjoint's 8-wide bf16 form: fs * a + (1 - fs) * v and w0 * r + w1 * r2
// each leave the compiler a choice of which product to fuse into the add, hipcc makes it per element of the unrolled group (in the 4-wide
// interpolation two elements get an fma and two a mul, mul, add), and an 8-wide body gets other choices: it differed from fuse_pool_kernel in
// the last bit of some outputs.  Bit equality with the existing kernel is what lets a mask of zeros stand for "no mask", so the body keeps
// fuse_pool_kernel's shape and with it 8-byte bf16 accesses.
template <typename T>
__global__ void fuse_pool_rows_kernel(const T* __restrict__ a_in, int Ta, const T* __restrict__ v_in, int Tv, const T* __restrict__ pe, int P,
                                      const int* __restrict__ mode, T* __restrict__ out, int L, int S_out, int D, float fs) {
    const int b = blockIdx.y, i = blockIdx.x;
    const int m = mode[b];
    const T* a = m == 2 ? nullptr : a_in;
    const T* v = m == 1 ? nullptr : v_in;
    const int Lt = P + L;
    for (int c = (int)threadIdx.x * FWD_VEC; c < D; c += (int)blockDim.x * FWD_VEC) {
        float acc[FWD_VEC], r[FWD_VEC];
#pragma unroll
        for (int k = 0; k < FWD_VEC; ++k) acc[k] = 0.f;
        if (Lt == S_out) {
            virt_row_n<T>(a, Ta, v, Tv, pe, P, b, i, c, D, fs, acc);
        } else if (Lt > S_out) {          // AdaptiveAvgPool1d window
            const int s = (int)(((long)i * Lt) / S_out);
            const int e = (int)((((long)(i + 1)) * Lt + S_out - 1) / S_out);
            for (int j = s; j < e; ++j) {
                virt_row_n<T>(a, Ta, v, Tv, pe, P, b, j, c, D, fs, r);
#pragma unroll
                for (int k = 0; k < FWD_VEC; ++k) acc[k] += r[k];
            }
            const float cnt = (float)(e - s);
#pragma unroll
            for (int k = 0; k < FWD_VEC; ++k) acc[k] = acc[k] / cnt;
        } else {                          // linear, align_corners=True
            const float scale = S_out > 1 ? (float)(Lt - 1) / (float)(S_out - 1) : 0.f;
            const float src = scale * i;
            const int lo = (int)src;
            const int hi = lo + 1 < Lt ? lo + 1 : Lt - 1;
            const float w1 = src - (float)lo, w0 = 1.0f - w1;
            float r2[FWD_VEC];
            virt_row_n<T>(a, Ta, v, Tv, pe, P, b, lo, c, D, fs, r);
            virt_row_n<T>(a, Ta, v, Tv, pe, P, b, hi, c, D, fs, r2);
#pragma unroll
            for (int k = 0; k < FWD_VEC; ++k) acc[k] = w0 * r[k] + w1 * r2[k];
        }
        store_f<FWD_VEC>(out + ((long)b * S_out + i) * D + c, acc);
    }
}

// ---------------------------------------------------------------- adjoint
// fuse_pool_bwd_kernel with the row's mode deciding the scales: block (t, b) gathers the dx rows that name virtual row P + t in ascending i
// (fp32, no atomics), then writes fs / 1 - fs (mode 0), 1 / 0 (mode 1) or 0 / 1 (mode 2) times the sum to da / dv.  Every row of both outputs
// is written: the unused stream's rows and rows t >= L are zeros.
template <typename T, int VEC>
__global__ void fuse_pool_rows_bwd_kernel(const T* __restrict__ dx, T* __restrict__ da, int Ta, T* __restrict__ dv, int Tv, int P,
                                          const int* __restrict__ mode, int L, int S_out, int D, float fs) {
    const int b = blockIdx.y, t = blockIdx.x;
    const int m = mode[b];
    const int Lt = P + L, j = P + t;
    const float scale = (Lt < S_out && S_out > 1) ? (float)(Lt - 1) / (float)(S_out - 1) : 0.f;
    int i0 = 0, i1 = -1;                  // t >= L: the forward truncated this row, its gradient is zero
    if (t < L) {
        if (Lt == S_out) { i0 = i1 = j; }
        else if (Lt > S_out) {
            i0 = (int)(((long)j * S_out) / Lt);
            i1 = (int)((((long)(j + 1)) * S_out - 1) / Lt);
        } else if (scale > 0.f) {
            i0 = (int)floorf((float)(j - 1) / scale) - 1;
            i1 = (int)ceilf((float)(j + 1) / scale) + 1;
        } else { i0 = 0; i1 = S_out - 1; }
        i0 = i0 < 0 ? 0 : i0;
        i1 = i1 > S_out - 1 ? S_out - 1 : i1;
    }
    for (int c = (int)threadIdx.x * VEC; c < D; c += (int)blockDim.x * VEC) {
        float g[VEC], r[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) g[k] = 0.f;
        for (int i = i0; i <= i1; ++i) {
            const T* src = dx + ((long)b * S_out + i) * D + c;
            if (Lt == S_out) {
                load_f<VEC>(src, g);
            } else if (Lt > S_out) {
                const int s = (int)(((long)i * Lt) / S_out);
                const int e = (int)((((long)(i + 1)) * Lt + S_out - 1) / S_out);
                if (j < s || j >= e) continue;
                const float cnt = (float)(e - s);
                load_f<VEC>(src, r);
#pragma unroll
                for (int k = 0; k < VEC; ++k) g[k] += r[k] / cnt;
            } else {
                const float sp = scale * i;
                const int lo = (int)sp;
                const int hi = lo + 1 < Lt ? lo + 1 : Lt - 1;
                if (lo != j && hi != j) continue;
                const float w1 = sp - (float)lo, w0 = 1.0f - w1;
                const float wgt = (lo == j ? w0 : 0.f) + (hi == j ? w1 : 0.f);
                load_f<VEC>(src, r);
#pragma unroll
                for (int k = 0; k < VEC; ++k) g[k] += wgt * r[k];
            }
        }
        if (t < Ta) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) r[k] = m == 2 ? 0.f : (m == 1 ? g[k] : fs * g[k]);
            store_f<VEC>(da + ((long)b * Ta + t) * D + c, r);
        }
        if (t < Tv) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) r[k] = m == 1 ? 0.f : (m == 2 ? g[k] : (1.0f - fs) * g[k]);
            store_f<VEC>(dv + ((long)b * Tv + t) * D + c, r);
        }
    }
}

// ---------------------------------------------------------------- draw
// One thread per clip; the whole rule is in include/avllm.h (avllm_modality_draw) and restated on the host by the tests.
__global__ void modality_draw_kernel(const int* mode_in, int* mode_out, int B, uint32_t ta, uint32_t tv, uint32_t seed, const uint32_t* seed_dev) {      // mode_out may alias mode_in
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int given = mode_in ? mode_in[b] : 0;
    int m = given;
    if (given != 1 && given != 2) {
        const uint32_t s = av_seed(seed_dev, seed) + 0x6D6F6461u;
        const uint32_t u = av_pair_hash(s, (unsigned long long)b) >> 8;
        m = u < ta ? 2 : (u >= (1u << 24) - tv ? 1 : 0);
    }
    mode_out[b] = m;
}

static inline int bwd_vec(int dtype, int D) { return dtype == AV_BF16 && D % 8 == 0 ? 8 : 4; }      // the adjoint, as fuse_pool_bwd: bf16 rows of whole 16-byte vectors take them

int av_fuse_pool_rows(const void* a, int Ta, const void* v, int Tv, const void* prompt_emb, int P, const int* mode, void* out, int B, int L,
                      int S_out, int D, float fs, int dtype, hipStream_t st) {
    AV_CHECK_ARG(a && v && mode, "fuse_pool_rows: needs both inputs and the modes (a %s, v %s, mode %s)", a ? "set" : "NULL", v ? "set" : "NULL", mode ? "set" : "NULL");
    AV_CHECK_ARG(out && B > 0 && L > 0 && S_out > 0 && Ta > 0 && Tv > 0 && P >= 0 && D > 0 && D % 4 == 0, "fuse_pool_rows: bad args (B=%d L=%d S_out=%d Ta=%d Tv=%d P=%d D=%d)", B, L, S_out, Ta, Tv, P, D);
    AV_CHECK_ARG(P == 0 || prompt_emb, "fuse_pool_rows: P>0 needs prompt_emb");
    AV_CHECK_ARG(dtype == AV_F32 || dtype == AV_BF16, "fuse_pool_rows: dtype %d", dtype);
    const dim3 grid(S_out, B), block(D / FWD_VEC < 256 ? (D / FWD_VEC + 63) / 64 * 64 : 256);
    if (dtype == AV_F32) hipLaunchKernelGGL((fuse_pool_rows_kernel<float>), grid, block, 0, st, (const float*)a, Ta, (const float*)v, Tv, (const float*)prompt_emb, P, mode, (float*)out, L, S_out, D, fs);
    else hipLaunchKernelGGL((fuse_pool_rows_kernel<bf16>), grid, block, 0, st, (const bf16*)a, Ta, (const bf16*)v, Tv, (const bf16*)prompt_emb, P, mode, (bf16*)out, L, S_out, D, fs);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_fuse_pool_rows_bwd(const void* dx, void* da, int Ta, void* dv, int Tv, int P, const int* mode, int B, int L, int S_out, int D, float fs,
                          int dtype, hipStream_t st) {
    AV_CHECK_ARG(dx && da && dv && mode, "fuse_pool_rows_bwd: needs dx, both outputs and the modes");
    AV_CHECK_ARG(B > 0 && L > 0 && S_out > 0 && Ta > 0 && Tv > 0 && P >= 0 && D > 0 && D % 4 == 0, "fuse_pool_rows_bwd: bad args (B=%d L=%d S_out=%d Ta=%d Tv=%d P=%d D=%d)", B, L, S_out, Ta, Tv, P, D);
    AV_CHECK_ARG(dtype == AV_F32 || dtype == AV_BF16, "fuse_pool_rows_bwd: dtype %d", dtype);
    const int vec = bwd_vec(dtype, D);
    const dim3 grid(Ta > Tv ? Ta : Tv, B), block(D / vec < 256 ? (D / vec + 63) / 64 * 64 : 256);
    if (dtype == AV_F32) hipLaunchKernelGGL((fuse_pool_rows_bwd_kernel<float, 4>), grid, block, 0, st, (const float*)dx, (float*)da, Ta, (float*)dv, Tv, P, mode, L, S_out, D, fs);
    else if (vec == 8) hipLaunchKernelGGL((fuse_pool_rows_bwd_kernel<bf16, 8>), grid, block, 0, st, (const bf16*)dx, (bf16*)da, Ta, (bf16*)dv, Tv, P, mode, L, S_out, D, fs);
    else hipLaunchKernelGGL((fuse_pool_rows_bwd_kernel<bf16, 4>), grid, block, 0, st, (const bf16*)dx, (bf16*)da, Ta, (bf16*)dv, Tv, P, mode, L, S_out, D, fs);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_modality_draw(const int* mode_in, int* mode_out, int B, float p_drop_audio, float p_drop_video, uint32_t seed, const uint32_t* seed_dev,
                     hipStream_t st) {
    AV_CHECK_ARG(mode_out && B > 0, "modality_draw: bad args (B=%d)", B);
    AV_CHECK_ARG(p_drop_audio >= 0.f && p_drop_audio <= 1.f && p_drop_video >= 0.f && p_drop_video <= 1.f && p_drop_audio + p_drop_video <= 1.f,
                 "modality_draw: probabilities %g (audio) and %g (video) must lie in [0, 1] with a sum of at most 1", (double)p_drop_audio, (double)p_drop_video);
    const uint32_t ta = (uint32_t)((double)p_drop_audio * 16777216.0 + 0.5), tv = (uint32_t)((double)p_drop_video * 16777216.0 + 0.5);      // of the float arguments, in double: exact
    hipLaunchKernelGGL(modality_draw_kernel, dim3((B + 255) / 256), dim3(256), 0, st, mode_in, mode_out, B, ta, tv, seed, seed_dev);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
