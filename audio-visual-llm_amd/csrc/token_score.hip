// Token scores of generate(): the log-probability of one chosen token per row and the entropy of the row's distribution, HF's
// `output_scores` / `compute_transition_scores` (transformers generation/utils.py), in ONE pass over float32 logits [rows, V].
//
// row_scores, for row r with y = x[r] / temperature:
//   lse = log(sum_v exp(y[v])),   out_logprob[r] = y[tokens[r]] - lse,   out_entropy[r] = lse - sum_v p[v] * y[v]  (nats), p = exp(y - lse).
// One 1024-thread workgroup per row.  A thread streams its share as 16-byte vectors, four loads in flight, and keeps a running state
//   (m, s, t) = (max y, sum exp(y - m), sum exp(y - m) * (y - m))
// which it rescales when the maximum moves (the online max/sum of attn_decode1_kernel and beam.hip, with a third term): then
//   lse = m + log(s),   logprob = (y[tok] - m) - log(s),   entropy = log(s) - t / s,
// so nothing of the size of m enters the entropy.  States are merged by a shuffle butterfly inside the wave and in wave order through LDS:
// a fixed order, no atomics, so a result repeats bit for bit.  Entries of -inf (banned tokens, avllm_logits_process) are skipped: they add
// 0 to both sums, never 0 * -inf.  A chosen token that is -inf gives -inf; a row of nothing but -inf has m = -inf, s = 0 and gives NaN twice.
// logprobs mode (rows that are log-probabilities already, avllm_logits_process with log_softmax = 1): nothing is normalised,
// out_logprob[r] = x[r][tokens[r]] as it stands and out_entropy[r] = -sum_v exp(x[v]) * x[v].
#include "common.h"
#include "avllm_internal.h"

namespace {

constexpr int NT = 1024, NWV = NT / AV_WAVE, UNROLL = 4;
constexpr int MAX_V = 2048 * 256;                  // sample.hip's MAX_V: generate() scores what it can sample

struct State { float m, s, t; };

// add y to the state; y > -inf
__device__ __forceinline__ void fold(State& a, float y) {
    const float d = y - a.m, e = expf(d);
    a.s += e;
    a.t += e * d;
}
// move the state's maximum up to mn > a.m
__device__ __forceinline__ void raise(State& a, float mn) {
    if (a.m > -INFINITY) {
        const float d = a.m - mn, e = expf(d);
        a.t = e * (a.t + a.s * d);
        a.s *= e;
    }
    a.m = mn;
}
// symmetric in its arguments, so both sides of a butterfly step hold the same bits
__device__ __forceinline__ State merge(State a, State b) {
    const float M = fmaxf(a.m, b.m);
    if (!(M > -INFINITY)) return a;                                    // nothing on either side yet
    if (a.m < M) raise(a, M);
    if (b.m < M) raise(b, M);
    return State{M, a.s + b.s, a.t + b.t};
}

template <bool LOGPROBS>
__device__ __forceinline__ void take4(State& a, float& h, const f32x4& v, float temp) {
    if constexpr (LOGPROBS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) h += v[j] > -INFINITY ? expf(v[j]) * v[j] : 0.f;
    } else {
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = v[j] / temp;
        const float mn = fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3]));
        if (mn > a.m) raise(a, mn);
#pragma unroll
        for (int j = 0; j < 4; ++j) if (y[j] > -INFINITY) fold(a, y[j]);
    }
}
template <bool LOGPROBS>
__device__ __forceinline__ void take1(State& a, float& h, float x, float temp) {
    if constexpr (LOGPROBS) {
        h += x > -INFINITY ? expf(x) * x : 0.f;
    } else {
        const float y = x / temp;
        if (y > a.m) raise(a, y);
        if (y > -INFINITY) fold(a, y);
    }
}

template <bool LOGPROBS>
__global__ __launch_bounds__(NT) void row_scores_kernel(const float* __restrict__ logits, long ld, int V, const int64_t* __restrict__ tokens,
                                                        float temp, float* __restrict__ out_logprob, float* __restrict__ out_entropy) {
    __shared__ float red[4][NWV];
    const int row = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float* g = logits + (long)row * ld;
    State a{-INFINITY, 0.f, 0.f};
    float h = 0.f;                                                     // logprobs mode: sum exp(x) * x
    if (!LOGPROBS || out_entropy) {
        // head up to the first 16-byte boundary, vectors, tail
        const int head = min(V, (int)((4 - (((uintptr_t)g >> 2) & 3)) & 3));
        const int n4 = (V - head) >> 2, tail0 = head + 4 * n4;
        if (threadIdx.x < head) take1<LOGPROBS>(a, h, g[threadIdx.x], temp);
        if (threadIdx.x >= NT - (V - tail0)) take1<LOGPROBS>(a, h, g[tail0 + (NT - 1 - threadIdx.x)], temp);
        const f32x4* g4 = (const f32x4*)(g + head);
        const f32x4 none = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int i0 = threadIdx.x; i0 < n4; i0 += NT * UNROLL) {
            f32x4 v[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) { const int i = i0 + u * NT; v[u] = i < n4 ? g4[i] : none; }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) take4<LOGPROBS>(a, h, v[u], temp);
        }
        // wave butterfly (every lane ends with the wave's state), then the waves in order
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            if constexpr (LOGPROBS) h += __shfl_xor(h, o);
            else a = merge(a, State{__shfl_xor(a.m, o), __shfl_xor(a.s, o), __shfl_xor(a.t, o)});
        }
        if (lane == 0) { red[0][wv] = a.m; red[1][wv] = a.s; red[2][wv] = a.t; red[3][wv] = h; }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    int64_t tok = tokens ? tokens[row] : 0;
    tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);                      // clamped: the host checks the range only where that costs no sync
    if constexpr (LOGPROBS) {
        if (out_logprob) out_logprob[row] = tokens ? g[tok] : 0.f;
        if (out_entropy) {
            float e = 0.f;
            for (int w = 0; w < NWV; ++w) e += red[3][w];
            out_entropy[row] = -e;
        }
    } else {
        State r{red[0][0], red[1][0], red[2][0]};
        for (int w = 1; w < NWV; ++w) r = merge(r, State{red[0][w], red[1][w], red[2][w]});
        const float ls = logf(r.s);
        if (out_logprob) out_logprob[row] = tokens ? (g[tok] / temp - r.m) - ls : -(r.m + ls);
        if (out_entropy) {
            const float e = ls - r.t / r.s;
            out_entropy[row] = e < 0.f ? 0.f : e;                      // rounding below zero only; NaN (an all -inf row) stays NaN
        }
    }
}

}  // namespace

int av_row_scores(const void* logits, long ld, long rows, int V, const int64_t* tokens, float temperature, float* out_logprob, float* out_entropy,
                  int logprobs, int dtype, hipStream_t st) {
    AV_CHECK_ARG(logits && (out_logprob || out_entropy) && rows > 0 && V > 0 && ld >= V, "row_scores: bad args");
    AV_CHECK_ARG(rows < (1L << 31), "row_scores: %ld rows", rows);
    AV_CHECK_ARG(dtype == AV_F32 || dtype == AV_BF16, "row_scores: dtype");
    if (dtype != AV_F32) return av_set_error(AV_ERR_UNSUPPORTED, "row_scores: float32 logits only (generate() holds no others)");
    if (V > MAX_V) return av_set_error(AV_ERR_UNSUPPORTED, "row_scores: V = %d > %d", V, MAX_V);
    if (logprobs) {
        hipLaunchKernelGGL(row_scores_kernel<true>, dim3((unsigned)rows), dim3(NT), 0, st, (const float*)logits, ld, V, tokens, 1.0f, out_logprob,
                           out_entropy);
    } else {
        AV_CHECK_ARG(temperature > 0.f && temperature < INFINITY, "row_scores: temperature must be > 0 (got %g)", (double)temperature);
        hipLaunchKernelGGL(row_scores_kernel<false>, dim3((unsigned)rows), dim3(NT), 0, st, (const float*)logits, ld, V, tokens, temperature,
                           out_logprob, out_entropy);
    }
    AV_LAUNCH_CHECK();
    return AV_OK;
}
