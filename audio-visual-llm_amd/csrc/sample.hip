// Sampled decoding: one token per row from temperature -> top-k -> top-p -> softmax -> one draw, the warper chain HF's GenerationMixin
// applies with do_sample=True (clip_whisper_model.py:1326-1340; transformers TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper).
//
// One 1024-thread workgroup per row.  A scaled logit x = logit / t is handled as an order-preserving uint32 key; the kept set is always
// {key >= T} for one threshold key T, so ties with the boundary value are kept whole:
//   top-k : T_k = the k-th largest key (radix select on counts, digits of 11/11/10 bits);
//   top-p : T_p = the largest key t with M(>= t) >= top_p * Z, M = softmax mass over keys >= T_k, Z = M(>= T_k).  With top-k on and at most
//           SORT_CAP survivors, from the survivors compacted and sorted in LDS; otherwise (top-k off, or ties past the capacity) by a radix
//           select that carries the mass per digit bin.  In descending order this is the shortest prefix whose tail mass is <= 1 - top_p,
//           plus every token whose scaled logit equals that of the last kept one.
//   draw  : inverse CDF over the kept tokens in vocabulary-index order, u = 24-bit hash of (seed [+ row_seeds[r]], step).
// Masses are fixed-point integers (exp(x - max) * 2^40, summed in uint64), so every histogram, scan and total is exact: the result repeats
// bit for bit whatever the order the threads add in, and no float atomic is used.  top_k == 1 is the argmax with argmax_kernel's rule
// (lowest index among equal maxima, temperature irrelevant).  NaN follows that rule in every mode: to_key reads a NaN of either sign as -inf,
// so it is never the maximum, carries no mass and is never drawn; a row of nothing but NaN and -inf returns token 0, as argmax_kernel does.
// out_logprob (optional): the draw's log-probability under the distribution it was drawn from, HF's transition score of a sampled token:
// (x_id - max) - log(W * 2^-40), W the exact kept mass the draw already holds; 0 where the kernel returns the argmax or pad.  One thread
// computes it after the draw: a null pointer leaves every pass, the LDS layout and the draws as they are.
// Rows of at most LDS_MAX_V entries are read from HBM once into LDS as keys; longer rows (Llama-3's 128,256) re-read the row, from L2, each pass.
#include "common.h"
#include "avllm_internal.h"

namespace {

constexpr int NT = 1024, NWV = NT / AV_WAVE;
constexpr int HB = 2048;                           // histogram bins of one radix pass (11-bit digit)
constexpr int SORT_CAP = HB;                       // top-k survivors sorted in the histogram's LDS
constexpr int TILE = 256;                          // draw pass: one wave sums 256 consecutive entries
constexpr int MAX_V = HB * TILE;                   // tile sums fit the histogram's LDS
constexpr int LDS_FIXED = HB * 8 + 2 * NWV * 8 + 16;
constexpr int LDS_MAX_V = (160 * 1024 - LDS_FIXED) / 4 / 16 * 16;

__device__ __forceinline__ uint32_t to_key(float x) {
    const uint32_t u = __float_as_uint(x == x ? x + 0.0f : -INFINITY);   // -0 -> +0: equal values, equal keys (argmax_kernel compares floats); NaN -> -inf
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_key(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ uint64_t mass(uint32_t k, float xmax) { return (uint64_t)(expf(from_key(k) - xmax) * 0x1p40f); }

template <typename T, bool IN_LDS> struct Row {
    const T* g; const uint32_t* s; float t;
    __device__ __forceinline__ uint32_t key(int i) const {
        if constexpr (IN_LDS) return s[i];
        else return to_key(to_f(g[i]) / t);
    }
};

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint64_t wave_max64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint64_t w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}
// inclusive block scan in thread order; red holds NWV entries; every thread gets the total
__device__ __forceinline__ uint64_t block_scan64(uint64_t v, uint64_t* red, uint64_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint64_t o = __shfl_up(v, d); if (lane >= d) v += o; }
    __syncthreads();
    if (lane == 63) red[w] = v;
    __syncthreads();
    uint64_t pre = 0, tot = 0;
    for (int i = 0; i < NWV; ++i) { pre += i < w ? red[i] : 0; tot += red[i]; }
    total = tot;
    return v + pre;
}

// Largest key t (>= floor) with A(>= t) >= target, A summing 1 per key (count) or its mass over the keys >= floor.  mass_p > 0: the target is
// ceil(mass_p * Z), Z = A(>= floor), known after the first pass.  *kept = A(>= t).
template <class R>
__device__ uint32_t radix_select(const R& r, int V, uint32_t floor, bool by_mass, float xmax, uint64_t target, float mass_p,
                                 uint64_t* hist, uint64_t* red, uint64_t* bc, uint64_t* kept) {
    uint32_t prefix = 0;
    uint64_t above = 0;
    for (int pass = 0; pass < 3; ++pass) {
        const int sh = pass == 0 ? 21 : (pass == 1 ? 10 : 0), hs = pass == 0 ? 32 : (pass == 1 ? 21 : 10);
        const uint32_t dmask = pass == 2 ? 1023u : 2047u;
        for (int b = threadIdx.x; b < HB; b += NT) hist[b] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < V; i += NT) {
            const uint32_t k = r.key(i);
            if (k < floor || (hs < 32 && (k >> hs) != (prefix >> hs))) continue;
            const uint64_t w = by_mass ? mass(k, xmax) : 1;
            if (w) atomicAdd((unsigned long long*)&hist[(k >> sh) & dmask], (unsigned long long)w);
        }
        __syncthreads();
        const int d0 = HB - 1 - 2 * threadIdx.x, d1 = d0 - 1;      // thread t owns two bins, in descending digit order
        const uint64_t b0 = hist[d0], b1 = hist[d1];
        uint64_t tot;
        const uint64_t inc = block_scan64(b0 + b1, red, tot), exc = inc - b0 - b1;
        if (pass == 0 && mass_p > 0.f) {
            const double tg = ceil((double)mass_p * (double)tot);
            target = tg < 1.0 ? 1 : (tg > (double)tot ? tot : (uint64_t)tg);
        }
        const uint64_t rt = target - above;
        if (threadIdx.x == 0) { bc[0] = 0; bc[1] = 0; bc[2] = 0; }
        __syncthreads();
        if (exc < rt && rt <= inc) {
            const bool first = exc + b0 >= rt;
            bc[0] = first ? d0 : d1; bc[1] = first ? exc : exc + b0; bc[2] = first ? b0 : b1;
        }
        __syncthreads();
        prefix |= (uint32_t)bc[0] << sh;
        above += bc[1];
        if (pass == 2) *kept = above + bc[2];
        __syncthreads();
    }
    return prefix;
}

template <typename T, bool IN_LDS>
__global__ __launch_bounds__(NT) void sample_kernel(const T* __restrict__ logits, long ld, int V, float temp, int top_k, float top_p,
                                                    uint32_t seed, const uint32_t* __restrict__ row_seeds, int step,
                                                    const int* __restrict__ step_dev, uint8_t* __restrict__ unfinished, long long eos,
                                                    long long pad, int64_t* __restrict__ out, float* __restrict__ out_logprob) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int row = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (unfinished && !unfinished[row]) {
        if (threadIdx.x == 0) { out[row] = pad; if (out_logprob) out_logprob[row] = 0.f; }
        return;
    }
    uint32_t* keys = (uint32_t*)smem;
    uint64_t* hist = (uint64_t*)(smem + (IN_LDS ? ((size_t)V * 4 + 15) / 16 * 16 : 0));
    uint64_t* red = hist + HB;
    uint64_t* bc = red + NWV;
    if (top_k == 1) temp = 1.0f;
    const T* g = logits + (long)row * ld;

    // pass 0: max key (lowest index among equal maxima) and, for short rows, the keys into LDS
    uint64_t best = 0;
    for (int i = threadIdx.x; i < V; i += NT) {
        const uint32_t k = to_key(to_f(g[i]) / temp);
        if constexpr (IN_LDS) keys[i] = k;
        const uint64_t c = ((uint64_t)k << 32) | (0xffffffffu - (uint32_t)i);
        best = c > best ? c : best;
    }
    best = wave_max64(best);
    if (lane == 0) red[wv] = best;
    __syncthreads();
    for (int i = 0; i < NWV; ++i) best = red[i] > best ? red[i] : best;
    __syncthreads();
    const uint32_t kmax = (uint32_t)(best >> 32);
    const float xmax = from_key(kmax);
    int64_t id = (int64_t)(0xffffffffu - (uint32_t)best);
    float lp = 0.f;                                    // log-probability of the draw; the argmax paths return their token with probability one
    const Row<T, IN_LDS> r{g, keys, temp};

    if (top_k != 1 && xmax > -INFINITY && xmax < INFINITY) {
        uint32_t thr = 0;
        uint64_t kept = 0;
        const bool use_k = top_k > 0 && top_k < V, use_p = top_p < 1.0f;
        if (use_k) thr = radix_select(r, V, 0u, false, xmax, (uint64_t)top_k, 0.f, hist, red, bc, &kept);
        if (use_p && use_k && kept <= (uint64_t)SORT_CAP) {
            // compact the top-k survivors (ties included) as (key, ~index), sort descending, scan their masses in that order
            const int n = (int)kept;
            int P = 64;
            while (P < n) P <<= 1;
            uint32_t* cnt = (uint32_t*)(bc + 3);
            for (int j = threadIdx.x; j < P; j += NT) hist[j] = 0;
            if (threadIdx.x == 0) *cnt = 0;
            __syncthreads();
            for (int i = threadIdx.x; i < V; i += NT) {
                const uint32_t k = r.key(i);
                if (k >= thr) hist[atomicAdd(cnt, 1u)] = ((uint64_t)k << 32) | (0xffffffffu - (uint32_t)i);
            }
            __syncthreads();
            for (int size = 2; size <= P; size <<= 1)
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int i = threadIdx.x; i < P / 2; i += NT) {
                        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                        const uint64_t a = hist[lo], b = hist[hi];
                        if ((a < b) == ((lo & size) == 0)) { hist[lo] = b; hist[hi] = a; }
                    }
                    __syncthreads();
                }
            const int j0 = 2 * threadIdx.x, j1 = j0 + 1;               // P <= 2 * NT
            const uint64_t w0 = j0 < n ? mass((uint32_t)(hist[j0] >> 32), xmax) : 0, w1 = j1 < n ? mass((uint32_t)(hist[j1] >> 32), xmax) : 0;
            uint64_t Z;
            const uint64_t s1 = block_scan64(w0 + w1, red, Z), s0 = s1 - w1;
            const double tg = ceil((double)top_p * (double)Z);
            const uint64_t target = tg < 1.0 ? 1 : (tg > (double)Z ? Z : (uint64_t)tg);
            if (threadIdx.x == 0) bc[0] = 0;
            __syncthreads();
            // first sorted position whose inclusive mass reaches the target: exactly one thread sees the crossing
            const uint64_t e0 = s0 - w0;
            if (j0 < n && e0 < target && s0 >= target) bc[0] = hist[j0] >> 32;
            if (j1 < n && s0 < target && s1 >= target) bc[0] = hist[j1] >> 32;
            __syncthreads();
            thr = (uint32_t)bc[0];
            __syncthreads();
        } else if (use_p) {
            thr = radix_select(r, V, thr, true, xmax, 0, top_p, hist, red, bc, &kept);
        }

        // draw: per-tile kept mass (index order), scan over tiles, then the crossing inside one tile
        const int ntile = (V + TILE - 1) / TILE;
        for (int t = wv; t < ntile; t += NWV) {
            uint64_t s = 0;
#pragma unroll
            for (int j = 0; j < TILE / 64; ++j) {
                const int i = t * TILE + j * 64 + lane;
                if (i < V) { const uint32_t k = r.key(i); if (k >= thr) s += mass(k, xmax); }
            }
            s = wave_sum64(s);
            if (lane == 0) hist[t] = s;
        }
        __syncthreads();
        const int t0 = 2 * threadIdx.x, t1 = t0 + 1;
        const uint64_t a0 = t0 < ntile ? hist[t0] : 0, a1 = t1 < ntile ? hist[t1] : 0;
        uint64_t W;
        const uint64_t inc = block_scan64(a0 + a1, red, W), exc = inc - a0 - a1;
        const uint32_t sr = seed + (row_seeds ? row_seeds[row] : 0u);
        const uint32_t st = (uint32_t)step + (step_dev ? (uint32_t)*step_dev : 0u);
        const uint32_t u24 = av_hash32(av_hash32(sr + 0x9E3779B9u) ^ st) >> 8;
        uint64_t target = (uint64_t)((double)W * ((double)u24 * 0x1p-24));
        target = target >= W ? W - 1 : target;
        if (threadIdx.x == 0) { bc[0] = 0; bc[1] = 0; }
        __syncthreads();
        if (exc <= target && target < inc) {
            const bool first = target < exc + a0;
            bc[0] = first ? t0 : t1; bc[1] = target - (first ? exc : exc + a0);
        }
        __syncthreads();
        if (wv == 0) {
            const int t = (int)bc[0];
            uint64_t rel = bc[1];
            for (int j = 0; j < TILE / 64; ++j) {
                const int i = t * TILE + j * 64 + lane;
                uint64_t w = 0;
                if (i < V) { const uint32_t k = r.key(i); if (k >= thr) w = mass(k, xmax); }
                uint64_t c = w;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const uint64_t o = __shfl_up(c, d); if (lane >= d) c += o; }
                const uint64_t hit = __ballot(c > rel);
                if (hit) { id = t * TILE + j * 64 + __ffsll((unsigned long long)hit) - 1; break; }
                rel -= __shfl(c, 63);
            }
            // the draw's log-probability under the kept, renormalised distribution: W is the kept mass in units of 2^-40 * exp(xmax)
            if (out_logprob && threadIdx.x == 0) lp = (from_key(r.key((int)id)) - xmax) - logf((float)W * 0x1p-40f);
        }
    }
    if (threadIdx.x == 0) {
        out[row] = id;
        if (out_logprob) out_logprob[row] = lp;
        if (unfinished && eos >= 0 && id == eos) unfinished[row] = 0;
    }
}

template <typename T, bool IN_LDS>
int launch(const void* logits, long ld, long rows, int V, float temp, int top_k, float top_p, uint32_t seed, const uint32_t* row_seeds,
           int step, const int* step_dev, uint8_t* unfinished, long long eos, long long pad, int64_t* out, float* out_logprob, hipStream_t st) {
    const size_t lds = IN_LDS ? ((size_t)V * 4 + 15) / 16 * 16 + LDS_FIXED : LDS_FIXED;
    if (IN_LDS) {
        static bool attr[64] = {};
        int dev = 0;
        AV_HIP(hipGetDevice(&dev));
        if (!attr[dev & 63]) {
            AV_HIP(hipFuncSetAttribute((const void*)sample_kernel<T, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       ((size_t)LDS_MAX_V * 4 + LDS_FIXED)));
            attr[dev & 63] = true;
        }
    }
    hipLaunchKernelGGL((sample_kernel<T, IN_LDS>), dim3(rows), dim3(NT), lds, st, (const T*)logits, ld, V, temp, top_k, top_p, seed, row_seeds,
                       step, step_dev, unfinished, eos, pad, out, out_logprob);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // namespace

int av_sample_rows(const void* logits, long ld, long rows, int V, float temperature, int top_k, float top_p, uint32_t seed,
                   const uint32_t* row_seeds, int step, const int* step_dev, uint8_t* unfinished, long long eos, long long pad,
                   int64_t* out, float* out_logprob, int dtype, hipStream_t st) {
    AV_CHECK_ARG(logits && out && rows > 0 && V > 0 && ld >= V, "sample_rows: bad args");
    AV_CHECK_ARG(temperature > 0.f && temperature < INFINITY, "sample_rows: temperature must be > 0 (got %g)", (double)temperature);
    AV_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "sample_rows: top_p must be in (0, 1] (got %g)", (double)top_p);
    AV_CHECK_ARG(top_k >= 0, "sample_rows: top_k must be >= 0 (got %d)", top_k);
    AV_CHECK_ARG(dtype == AV_F32 || dtype == AV_BF16, "sample_rows: dtype");
    if (V > MAX_V) return av_set_error(AV_ERR_UNSUPPORTED, "sample_rows: V = %d > %d", V, MAX_V);
    const bool in_lds = V <= LDS_MAX_V;
    if (dtype == AV_F32)
        return in_lds ? launch<float, true>(logits, ld, rows, V, temperature, top_k, top_p, seed, row_seeds, step, step_dev, unfinished, eos, pad, out, out_logprob, st)
                      : launch<float, false>(logits, ld, rows, V, temperature, top_k, top_p, seed, row_seeds, step, step_dev, unfinished, eos, pad, out, out_logprob, st);
    return in_lds ? launch<bf16, true>(logits, ld, rows, V, temperature, top_k, top_p, seed, row_seeds, step, step_dev, unfinished, eos, pad, out, out_logprob, st)
                  : launch<bf16, false>(logits, ld, rows, V, temperature, top_k, top_p, seed, row_seeds, step, step_dev, unfinished, eos, pad, out, out_logprob, st);
}
