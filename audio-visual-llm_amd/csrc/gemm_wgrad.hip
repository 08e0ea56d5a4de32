// Weight gradient of a Linear:  dW[n,k] = alpha * sum_m dY[m,n] * X[m,k],  db[n] = alpha * sum_m dY[m,n]   (autograd of nn.Linear; the
// trainable modality connectors, reference modality_connector.py:25-44).  gemm_tn.hip does this product for a 16-column small operand with
// float atomics over M-chunks; this is the general form, and it is deterministic: one workgroup owns a 128x128 output tile for the WHOLE of M
// (at the connector shapes, N = 4096 x K = 768: 32 x 6 = 192 tiles on 256 CUs, one round), db is a fixed-order column sum in a sibling launch.
// Both operands are row-major over the REDUCTION index m, i.e. k-strided for an MFMA: both go through LDS as they lie in memory and come
// back as fragments with ds_read_b64_tr_b16 (hardware transpose), as in gemm_tn.hip.
#include "common.h"
#include "avllm_internal.h"

namespace {

typedef __attribute__((address_space(3))) short4v* lds_s4_ptr;
typedef __attribute__((ext_vector_type(8))) short short8v;

// 16x16x32 operand whose k index runs over LDS tile rows [row0, row0+32) and whose 16 rows/cols are tile columns col0..col0+15
__device__ __forceinline__ bf16x8 tr_frag16(const char* img, int stride, int row0, int col0, int lane) {
    const int g = lane >> 4, i16 = lane & 15;
    const char* a0 = img + (row0 + 8 * g + (i16 >> 2)) * stride + (col0 + 4 * (i16 & 3)) * 2;
    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)(a0));
    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)(a0 + 4 * stride));
    const short8v both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, both);
}

// The epilogue's value: alpha * acc, rounded, and with ACC the cell's prior value added to it in a second rounding (the pragma keeps the compiler
// from contracting the two into one fma: onto a prior 0 the result is then the overwriting form's bits for every input).
template <bool ACC> __device__ __forceinline__ void wgrad_store(float* cell, float alpha, float acc) {
#pragma clang fp contract(off)
    const float r = alpha * acc;
    *cell = ACC ? *cell + r : r;
}

constexpr int WG_T = 128, WG_M = 64;          // output tile 128 (n) x 128 (k); 64 rows of m per slab
constexpr int WG_STRIDE = WG_T * 2 + 64;      // 320 B: the 4 rows of a transposed read land on distinct bank quarters (gemm_tn.hip)
constexpr int WG_CHUNKS = WG_M * (WG_T / 8) / 256;       // 4 16-byte chunks of each operand per thread and slab

// 4 waves as 2 (n) x 2 (k), 64 x 64 outputs each = 4 x 4 MFMA tiles.  Ragged edges: rows m >= M and chunks past N / K are zero-filled
// (N, K multiples of 8: a chunk is in or out as a whole), stores past N / K are dropped.
// ACC (avllm_gemm_wgrad_acc): the epilogue adds the cell's prior value, read once after the K-loop through the same address the store uses
// (16 lanes x 4 B contiguous per row, 4 rows per instruction: the 64-byte segments the store already writes), in fp32, after the product with
// alpha.  The tile's owner is still one workgroup for the whole of M, so the sum needs no atomics.
template <bool ACC>
__global__ __launch_bounds__(256) void wgrad_bf16_kernel(const bf16* __restrict__ dY, long ldy, const bf16* __restrict__ X, long ldx, int M,
                                                         int N, int K, float* __restrict__ dW, long ldw, float alpha) {
    __shared__ __attribute__((aligned(16))) char ys[WG_M * WG_STRIDE];
    __shared__ __attribute__((aligned(16))) char xs[WG_M * WG_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n0 = blockIdx.x * WG_T, k0 = blockIdx.y * WG_T;
    const int wn = (w >> 1) * 64, wk = (w & 1) * 64;
    f32x4 acc[4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // software pipeline: the next slab travels global -> registers while the MFMAs of the current one run
    u32x4 ry[WG_CHUNKS], rx[WG_CHUNKS];
    auto fetch = [&](int mb) {
#pragma unroll
        for (int i = 0; i < WG_CHUNKS; ++i) {
            const int c = tid + i * 256, row = c >> 4, ch = c & 15;
            ry[i] = (u32x4){0u, 0u, 0u, 0u};
            rx[i] = (u32x4){0u, 0u, 0u, 0u};
            if (mb + row < M) {
                if (n0 + ch * 8 < N) ry[i] = *(const u32x4*)(dY + (long)(mb + row) * ldy + n0 + ch * 8);
                if (k0 + ch * 8 < K) rx[i] = *(const u32x4*)(X + (long)(mb + row) * ldx + k0 + ch * 8);
            }
        }
    };
    fetch(0);
    for (int mb = 0; mb < M; mb += WG_M) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < WG_CHUNKS; ++i) {
            const int c = tid + i * 256, row = c >> 4, ch = c & 15;
            *(u32x4*)(ys + row * WG_STRIDE + ch * 16) = ry[i];
            *(u32x4*)(xs + row * WG_STRIDE + ch * 16) = rx[i];
        }
        __syncthreads();
        if (mb + WG_M < M) fetch(mb + WG_M);
#pragma unroll
        for (int ks = 0; ks < WG_M / 32; ++ks) {
            bf16x8 a[4], b[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) a[x] = tr_frag16(ys, WG_STRIDE, 32 * ks, wn + 16 * x, lane);      // A: rows n, k index = m
#pragma unroll
            for (int y = 0; y < 4; ++y) b[y] = tr_frag16(xs, WG_STRIDE, 32 * ks, wk + 16 * y, lane);      // B: k index = m, cols k
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[x], b[y], acc[x][y], 0, 0, 0);      // D[n][k]
        }
    }
    const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int k = k0 + wk + 16 * y + fr;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + wn + 16 * x + fq * 4 + i;
                if (n < N && k < K) wgrad_store<ACC>(dW + (long)n * ldw + k, alpha, acc[x][y][i]);
            }
        }
}

// fp32 (parity mode): 64 x 64 outputs per block, 4 x 4 per thread, plain fp32 FMAs in ascending m
template <bool ACC>
__global__ __launch_bounds__(256) void wgrad_f32_kernel(const float* __restrict__ dY, long ldy, const float* __restrict__ X, long ldx, int M, int N,
                                                        int K, float* __restrict__ dW, long ldw, float alpha) {
    __shared__ float Ys[32][65], Xs[32][65];
    const int n0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
    const int tn = threadIdx.x >> 4, tk = threadIdx.x & 15;
    float acc[4][4] = {};
    for (int mb = 0; mb < M; mb += 32) {
        __syncthreads();
        for (int e = threadIdx.x; e < 32 * 64; e += 256) {
            const int mm = e >> 6, c = e & 63, m = mb + mm;
            Ys[mm][c] = (m < M && n0 + c < N) ? dY[(long)m * ldy + n0 + c] : 0.f;
            Xs[mm][c] = (m < M && k0 + c < K) ? X[(long)m * ldx + k0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int mm = 0; mm < 32; ++mm) {
            float a[4], b[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) { a[x] = Ys[mm][tn * 4 + x]; b[x] = Xs[mm][tk * 4 + x]; }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[x][y] += a[x] * b[y];
        }
    }
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int n = n0 + tn * 4 + x, k = k0 + tk * 4 + y;
            if (n < N && k < K) wgrad_store<ACC>(dW + (long)n * ldw + k, alpha, acc[x][y]);
        }
}

// db[n] = alpha * sum_m dY[m,n]: a block owns 64 columns (8 chunks of 8) for the whole of M; 32 row groups each add their rows m = g, g + 32, ...
// in ascending order, then one thread per column adds the 32 partials in group order.
template <typename T, bool ACC>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ dY, long ldy, int M, int N, float* __restrict__ db, float alpha) {
    __shared__ float part[32][65];
    const int ch = threadIdx.x & 7, rg = threadIdx.x >> 3;
    const int n = blockIdx.x * 64 + ch * 8;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, r[8];
    if (n < N)
        for (int m = rg; m < M; m += 32) {
            load_f<8>(dY + (long)m * ldy + n, r);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += r[j];
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) part[rg][ch * 8 + j] = s[j];
    __syncthreads();
    if (threadIdx.x < 64 && blockIdx.x * 64 + (int)threadIdx.x < N) {
        float t = 0.f;
        for (int g = 0; g < 32; ++g) t += part[g][threadIdx.x];
        wgrad_store<ACC>(db + blockIdx.x * 64 + threadIdx.x, alpha, t);
    }
}

}  // namespace

template <bool ACC>
static int wgrad_launch(const void* dY, long ldy, const void* X, long ldx, int M, int N, int K, float* dW, long ldw, float* db, float alpha, int dtype,
                        hipStream_t st) {
    AV_CHECK_ARG(dY && X && dW && M >= 1 && N >= 1 && K >= 1, "gemm_wgrad: null / empty (M=%d N=%d K=%d)", M, N, K);
    AV_CHECK_ARG(dtype == AV_F32 || dtype == AV_BF16, "gemm_wgrad: dtype %d", dtype);
    AV_CHECK_ARG(N % 8 == 0 && K % 8 == 0 && ldy % 8 == 0 && ldx % 8 == 0 && ldy >= N && ldx >= K && ldw >= K,
                 "gemm_wgrad: N=%d K=%d ldy=%ld ldx=%ld must be multiples of 8 (16-byte operand chunks), ldw=%ld >= K", N, K, ldy, ldx, ldw);
    AV_CHECK_ARG((((uintptr_t)dY | (uintptr_t)X) & 15) == 0, "gemm_wgrad: dY and X must be 16-byte aligned (the operands are read as 16-byte chunks)");
    if (dtype == AV_BF16)
        hipLaunchKernelGGL(wgrad_bf16_kernel<ACC>, dim3(av_cdiv(N, WG_T), av_cdiv(K, WG_T)), dim3(256), 0, st, (const bf16*)dY, ldy, (const bf16*)X, ldx,
                           M, N, K, dW, ldw, alpha);
    else
        hipLaunchKernelGGL(wgrad_f32_kernel<ACC>, dim3(av_cdiv(N, 64), av_cdiv(K, 64)), dim3(256), 0, st, (const float*)dY, ldy, (const float*)X, ldx, M,
                           N, K, dW, ldw, alpha);
    if (db) {
        if (dtype == AV_BF16) hipLaunchKernelGGL((colsum_kernel<bf16, ACC>), dim3(av_cdiv(N, 64)), dim3(256), 0, st, (const bf16*)dY, ldy, M, N, db, alpha);
        else hipLaunchKernelGGL((colsum_kernel<float, ACC>), dim3(av_cdiv(N, 64)), dim3(256), 0, st, (const float*)dY, ldy, M, N, db, alpha);
    }
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_gemm_wgrad(const void* dY, long ldy, const void* X, long ldx, int M, int N, int K, float* dW, long ldw, float* db, float alpha, int dtype,
                  hipStream_t st) {
    return wgrad_launch<false>(dY, ldy, X, ldx, M, N, K, dW, ldw, db, alpha, dtype, st);
}

int av_gemm_wgrad_acc(const void* dY, long ldy, const void* X, long ldx, int M, int N, int K, float* dW, long ldw, float* db, float alpha, int dtype,
                      hipStream_t st) {
    return wgrad_launch<true>(dY, ldy, X, ldx, M, N, K, dW, ldw, db, alpha, dtype, st);
}
