// Per-head RMSNorm of q and k fused with the rotary embedding (Qwen3: transformers/models/qwen3/modeling_qwen3.py Qwen3Attention.forward,
// q_norm(q_proj(x).view(.., hd)) / k_norm(..) then apply_rotary_pos_emb), and its backward.  Both work in place on the adjacent q and k
// slices of a [M, ld] q|k|v buffer; v is never written.
//
// Layout.  A head is hd elements of one row; the rotary partner of element i is i + hd/2, so a lane takes 16 bytes of the first half and
// the 16 bytes at the same offset of the second half: L = hd/2 / (16 / sizeof(T)) lanes own a head (bf16: 4 for hd 64, 8 for hd 128; fp32:
// 8 and 16), a wave 64 / L whole heads.  Every load and store is 16 bytes per lane; the sum of squares (backward: of g * xhat) is a
// butterfly over the L lanes of the group (__shfl_xor, offsets < L stay inside the group); no LDS.  HBM-bound: a head is read once and
// written once, the weight vectors and the table stay in L2.  All arithmetic is fp32 and the result is rounded once.
#include "common.h"
#include "avllm_internal.h"

namespace {

struct QkNormArgs {
    void* x; long ld; long M; int T_, H, Hkv, hd;
    const void *wq, *wk; float eps;
    const float* tab;                   // [T][hd/2][2] cos, sin; row r reads table row r % T
    void* pre; float* rstd;             // optional saves: pre-norm q|k [M, (H+Hkv) hd], rstd [M, H+Hkv]
    void *kc, *vc; int Tmax, pos; const int* pos_dev;      // cache form (T == 1, row = sequence): k (rotated) and v go to cache row pos + *pos_dev
};

template <typename T, int N> __device__ __forceinline__ void load2(const T* p, int half, float (&a)[N], float (&b)[N]) {
    load_f<N>(p, a);
    load_f<N>(p + half, b);
}
template <typename T, int N> __device__ __forceinline__ void store2(T* p, int half, const float (&a)[N], const float (&b)[N]) {
    store_f<N>(p, a);
    store_f<N>(p + half, b);
}
// sum over the L lanes of a head's group (L = 4, 8 or 16: a power of two, groups are aligned inside the wave)
__device__ __forceinline__ float group_sum(float v, int L) {
    for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <typename T>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(QkNormArgs a) {
    constexpr int N = 16 / sizeof(T);
    const int half = a.hd >> 1, L = half / N;
    const int NQK = a.H + a.Hkv, NH = a.kc ? NQK + a.Hkv : NQK;
    const long gid = (blockIdx.x * (long)blockDim.x + threadIdx.x) / L;
    if (gid >= a.M * NH) return;                      // whole groups leave together
    const int c = (threadIdx.x % L) * N;
    const long row = gid / NH;
    const int h = (int)(gid - row * NH);
    T* p = (T*)a.x + row * a.ld + (long)h * a.hd + c;
    float xa[N], xb[N];
    load2<T, N>(p, half, xa, xb);
    // the position comes from device memory when the step is replayed from a graph: the host could not check it, so a row past the end of
    // the cache is not written (dec_proj and attn_decode1_kernel guard alike)
    const int pos = a.pos + (a.pos_dev ? *a.pos_dev : 0);
    const bool in_cache = pos >= 0 && pos < a.Tmax;
    const long dkv = (long)a.Hkv * a.hd;
    if (h >= NQK) {                                   // v head (cache form only): copied, untouched
        if (in_cache) store2<T, N>((T*)a.vc + (row * a.Tmax + pos) * dkv + (long)(h - NQK) * a.hd + c, half, xa, xb);
        return;
    }
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) ss += xa[i] * xa[i] + xb[i] * xb[i];
    ss = group_sum(ss, L);
    const float rs = rsqrtf(ss / (float)a.hd + a.eps);
    if (a.pre) store2<T, N>((T*)a.pre + (row * NQK + h) * a.hd + c, half, xa, xb);
    if (a.rstd && c == 0) a.rstd[row * NQK + h] = rs;
    float wa[N], wb[N], cs[2 * N], oa[N], ob[N];
    load2<T, N>((const T*)(h < a.H ? a.wq : a.wk) + c, half, wa, wb);
    load_f<2 * N>(a.tab + ((row % a.T_) * half + c) * 2, cs);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float ya = xa[i] * rs * wa[i], yb = xb[i] * rs * wb[i];
        oa[i] = ya * cs[2 * i] - yb * cs[2 * i + 1];
        ob[i] = yb * cs[2 * i] + ya * cs[2 * i + 1];
    }
    if (h < a.H || !a.kc) store2<T, N>(p, half, oa, ob);
    else if (in_cache) store2<T, N>((T*)a.kc + (row * a.Tmax + pos) * dkv + (long)(h - a.H) * a.hd + c, half, oa, ob);
}

// dx = rstd * (g - xhat * mean(g * xhat)), g = w * dy, xhat = x_pre * rstd; dy is the gradient with respect to the PRE-RoPE normed head
template <typename T>
__global__ __launch_bounds__(256) void qk_norm_bwd_kernel(T* __restrict__ dy, long ld, long M, int NQK, int H, int hd, const T* __restrict__ wq,
                                                          const T* __restrict__ wk, const T* __restrict__ pre, const float* __restrict__ rstd) {
    constexpr int N = 16 / sizeof(T);
    const int half = hd >> 1, L = half / N;
    const long gid = (blockIdx.x * (long)blockDim.x + threadIdx.x) / L;
    if (gid >= M * NQK) return;
    const int c = (threadIdx.x % L) * N;
    const long row = gid / NQK;
    const int h = (int)(gid - row * NQK);
    T* p = dy + row * ld + (long)h * hd + c;
    float ga[N], gb[N], xa[N], xb[N], wa[N], wb[N];
    load2<T, N>(p, half, ga, gb);
    load2<T, N>(pre + gid * hd + c, half, xa, xb);
    load2<T, N>((h < H ? wq : wk) + c, half, wa, wb);
    const float rs = rstd[gid];
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        ga[i] *= wa[i]; gb[i] *= wb[i];
        xa[i] *= rs; xb[i] *= rs;
        dot += ga[i] * xa[i] + gb[i] * xb[i];
    }
    const float mean = group_sum(dot, L) / (float)hd;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        ga[i] = rs * (ga[i] - xa[i] * mean);
        gb[i] = rs * (gb[i] - xb[i] * mean);
    }
    store2<T, N>(p, half, ga, gb);
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int av_qk_norm_rope(void* x, long ld, long M, int T, int H, int Hkv, int hd, const void* wq, const void* wk, float eps, const float* tab, void* pre,
                    float* rstd, void* kc, void* vc, int Tmax, int pos, const int* pos_dev, int dtype, hipStream_t st) {
    AV_CHECK_ARG(x && wq && wk && tab && M > 0 && T > 0 && H > 0 && Hkv > 0, "qk_norm_rope: null/empty");
    AV_CHECK_ARG(dtype == AV_F32 || dtype == AV_BF16, "qk_norm_rope: dtype %d", dtype);
    AV_CHECK_ARG(hd == 64 || hd == 128, "qk_norm_rope: head_dim %d (64 or 128)", hd);
    const int n16 = 16 / (int)av_dtype_size(dtype);
    const bool cache = kc || vc;
    AV_CHECK_ARG(ld % n16 == 0 && ld >= (long)(H + Hkv + (cache ? Hkv : 0)) * hd, "qk_norm_rope: rows of ld=%ld must be 16-byte multiples that hold the heads", ld);
    AV_CHECK_ARG(al16(x) && al16(wq) && al16(wk) && al16(tab) && al16(pre) && al16(kc) && al16(vc), "qk_norm_rope: 16-byte aligned pointers");
    AV_CHECK_ARG(!cache || (kc && vc && T == 1 && Tmax > 0 && pos >= 0 && (pos_dev || pos < Tmax)),
                 "qk_norm_rope(cache form): kc and vc, one position per row (T=%d), pos=%d inside the cache (Tmax=%d)", T, pos, Tmax);
    QkNormArgs a = {x, ld, M, T, H, Hkv, hd, wq, wk, eps, tab, pre, rstd, kc, vc, cache ? Tmax : 0, pos, cache ? pos_dev : nullptr};
    const long lanes = M * (H + Hkv + (cache ? Hkv : 0)) * (hd / 2 / n16);
    const dim3 grid(av_cdiv(lanes, 256));
    if (dtype == AV_F32) hipLaunchKernelGGL(qk_norm_rope_kernel<float>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(qk_norm_rope_kernel<bf16>, grid, dim3(256), 0, st, a);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_qk_norm_bwd(void* dy, long ld, long M, int H, int Hkv, int hd, const void* wq, const void* wk, const void* pre, const float* rstd, int dtype,
                   hipStream_t st) {
    AV_CHECK_ARG(dy && wq && wk && pre && rstd && M > 0 && H > 0 && Hkv > 0, "qk_norm_bwd: null/empty");
    AV_CHECK_ARG(dtype == AV_F32 || dtype == AV_BF16, "qk_norm_bwd: dtype %d", dtype);
    AV_CHECK_ARG(hd == 64 || hd == 128, "qk_norm_bwd: head_dim %d (64 or 128)", hd);
    const int n16 = 16 / (int)av_dtype_size(dtype);
    AV_CHECK_ARG(ld % n16 == 0 && ld >= (long)(H + Hkv) * hd, "qk_norm_bwd: rows of ld=%ld must be 16-byte multiples that hold the heads", ld);
    AV_CHECK_ARG(al16(dy) && al16(wq) && al16(wk) && al16(pre), "qk_norm_bwd: 16-byte aligned pointers");
    const long lanes = M * (H + Hkv) * (hd / 2 / n16);
    const dim3 grid(av_cdiv(lanes, 256));
    if (dtype == AV_F32) hipLaunchKernelGGL(qk_norm_bwd_kernel<float>, grid, dim3(256), 0, st, (float*)dy, ld, M, H + Hkv, H, hd, (const float*)wq, (const float*)wk, (const float*)pre, rstd);
    else hipLaunchKernelGGL(qk_norm_bwd_kernel<bf16>, grid, dim3(256), 0, st, (bf16*)dy, ld, M, H + Hkv, H, hd, (const bf16*)wq, (const bf16*)wk, (const bf16*)pre, rstd);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int avllm_qk_norm_rope(void* x, int64_t ld, int64_t rows, int32_t T, int32_t heads, int32_t kv_heads, int32_t hd, const void* q_norm_w,
                                  const void* k_norm_w, float eps, const float* tab, void* pre, float* rstd, void* kc, void* vc, int32_t Tmax, int32_t pos,
                                  const int32_t* pos_dev, int32_t dtype, void* stream) {
    return av_qk_norm_rope(x, ld, rows, T, heads, kv_heads, hd, q_norm_w, k_norm_w, eps, tab, pre, rstd, kc, vc, Tmax, pos, pos_dev, dtype, (hipStream_t)stream);
}
extern "C" int avllm_qk_norm_bwd(void* dy, int64_t ld, int64_t rows, int32_t heads, int32_t kv_heads, int32_t hd, const void* q_norm_w, const void* k_norm_w,
                                 const void* pre, const float* rstd, int32_t dtype, void* stream) {
    return av_qk_norm_bwd(dy, ld, rows, heads, kv_heads, hd, q_norm_w, k_norm_w, pre, rstd, dtype, (hipStream_t)stream);
}
