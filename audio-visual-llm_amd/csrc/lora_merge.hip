// Fold one LoRA pair into its frozen matrix, in place and once per load (LlamaEngine.merge_lora): W[n,k] <- round(W[n,k] + scale * u[n,k]),
// u[n,k] = sum_{j<r} B[n,j] * A[j,k].  After it the adapter-free prefill and token step compute the adapted model.
//
// Arithmetic (the contract tests/bars_merge.py derives its bar from): fp32 throughout from the fp32 masters; u is ONE fma chain over
// j = 0 .. r-1 in ascending order starting from 0; then one fma(scale, u, W) and one round-to-nearest-even to the storage type.  No atomics,
// no split of the rank sum across threads: two launches on equal inputs write equal bytes.
//
// Shape of the work: memory-bound (r <= 64 fma per element against one 16-byte read and write per 8 bf16 elements).  A block owns a strip
// of 128 columns: it stages the strip of A ([r, 128] f32, at most 32 KiB) in LDS once and walks row tiles of 64 rows down the strip, staging
// the tile's B rows ([64, r], row stride r|1 so that the four rows a wave reads at once fall on different banks) per tile.  A thread owns 8
// consecutive columns (one 16-byte access of bf16, two of f32) of 4 rows, so every ds_read_b128 of A serves 4 rows and the 16 lanes of a
// read group cover one 256-byte bank row; B values are wave broadcasts.  A tile's W rows are requested before the staging loads.  The grid is (K/128 strips) x (as many row walkers as give about
// four blocks per CU): 32 x 32 at N = K = 4096, 32 x 16 at a grouped-query N = 1024.
#include "common.h"
#include "avllm_internal.h"

namespace {

constexpr int LM_THREADS = 256;
constexpr int LM_TK = 128;        // columns of a strip: 16 column groups of 8
constexpr int LM_RPT = 4;         // rows per thread
constexpr int LM_TN = (LM_THREADS / 16) * LM_RPT;      // 64 rows of a row tile

template <typename T>
__global__ __launch_bounds__(LM_THREADS) void lora_merge_kernel(T* W, long ldw, int N, int K, const float* __restrict__ A,
                                                                const float* __restrict__ B, int r, float scale) {
    extern __shared__ float lm_smem[];
    float* As = lm_smem;                       // [r][LM_TK]
    const int bs = r | 1;
    float* Bs = lm_smem + r * LM_TK;           // [LM_TN][bs]
    const int t = threadIdx.x, cg = t & 15, rg = t >> 4;
    const int kt = blockIdx.x * LM_TK;
    const int k0 = kt + cg * 8;
    const bool live = k0 < K;                  // K % 8 == 0: a column group is inside the matrix or outside it as a whole
    // a tile's W rows are requested before the staging loads of A and B, so that the three latencies overlap
    float w[LM_RPT][8];
    auto load_w = [&](int nt) {
#pragma unroll
        for (int i = 0; i < LM_RPT; ++i) {
            const int n = nt + rg * LM_RPT + i;
            if (live && n < N) load_f<8>(W + (long)n * ldw + k0, w[i]);
        }
    };
    const int nt0 = blockIdx.y * LM_TN;        // < N: the grid has at most as many row walkers as row tiles
    load_w(nt0);
    // the masters carry no alignment promise (slices of one flat buffer): 4-byte loads, consecutive lanes on consecutive addresses
    for (int i = t; i < r * LM_TK; i += LM_THREADS) {
        const int j = i / LM_TK, k = kt + (i % LM_TK);
        As[i] = k < K ? A[(long)j * K + k] : 0.f;
    }
    for (int nt = nt0; nt < N; nt += gridDim.y * LM_TN) {
        if (nt != nt0) {
            __syncthreads();                   // the previous tile's reads of Bs are done
            load_w(nt);
        }
        const int rows = min(LM_TN, N - nt);
        for (int i = t; i < rows * r; i += LM_THREADS) Bs[(i / r) * bs + (i % r)] = B[(long)nt * r + i];
        __syncthreads();
        if (!live) continue;
        float u[LM_RPT][8];
#pragma unroll
        for (int i = 0; i < LM_RPT; ++i)
#pragma unroll
            for (int c = 0; c < 8; ++c) u[i][c] = 0.f;
        const float* ap = As + cg * 8;
        const float* bp = Bs + rg * LM_RPT * bs;       // rows past N hold stale values: their results are never stored
        for (int j = 0; j < r; ++j) {
            float a[8];
            load_f<8>(ap + j * LM_TK, a);
#pragma unroll
            for (int i = 0; i < LM_RPT; ++i) {
                const float b = bp[i * bs + j];
#pragma unroll
                for (int c = 0; c < 8; ++c) u[i][c] = fmaf(b, a[c], u[i][c]);
            }
        }
#pragma unroll
        for (int i = 0; i < LM_RPT; ++i) {
            const int n = nt + rg * LM_RPT + i;
            if (n >= N) continue;
#pragma unroll
            for (int c = 0; c < 8; ++c) w[i][c] = fmaf(scale, u[i][c], w[i][c]);
            store_f<8>(W + (long)n * ldw + k0, w[i]);
        }
    }
}

}  // namespace

int av_lora_merge(void* W, long ldw, int N, int K, const float* A, const float* B, int r, float scale, int dtype, hipStream_t st) {
    AV_CHECK_ARG(W && A && B, "lora_merge: null pointer");
    AV_CHECK_ARG(r >= 1 && r <= AVLLM_LORA_PAD, "lora_merge: rank %d outside 1..%d", r, AVLLM_LORA_PAD);
    AV_CHECK_ARG(N >= 1, "lora_merge: N=%d", N);
    AV_CHECK_ARG(K >= 8 && K % 8 == 0 && ldw % 8 == 0 && ldw >= K, "lora_merge: K=%d and ldw=%ld must be multiples of 8 with ldw >= K", K, (long)ldw);
    AV_CHECK_ARG(((uintptr_t)W & 15) == 0, "lora_merge: W must be 16-byte aligned");
    AV_CHECK_ARG(dtype == AV_F32 || dtype == AV_BF16, "lora_merge: dtype %d", dtype);
    if (scale == 0.f) return AV_OK;            // W + 0 * B.A = W: nothing to read or write (and a -0.0 in W keeps its sign)
    int ncu = 256;
    av_device(&ncu);
    const int strips = av_cdiv(K, LM_TK), tiles = av_cdiv(N, LM_TN);
    int walkers = av_cdiv(4L * ncu, strips);
    walkers = walkers < 1 ? 1 : walkers > tiles ? tiles : walkers;       // <= 4 * ncu: far below the grid's y limit
    const size_t lds = ((size_t)r * LM_TK + (size_t)LM_TN * (r | 1)) * sizeof(float);       // <= 49 KiB at r = 64: below the 64 KiB default limit
    const dim3 grid(strips, walkers), block(LM_THREADS);
    if (dtype == AV_BF16) hipLaunchKernelGGL((lora_merge_kernel<bf16>), grid, block, lds, st, (bf16*)W, ldw, N, K, A, B, r, scale);
    else hipLaunchKernelGGL((lora_merge_kernel<float>), grid, block, lds, st, (float*)W, ldw, N, K, A, B, r, scale);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
