// Beam-search decoding on the device: candidate selection (HF's `log_softmax` + `_get_top_k_continuations`, transformers
// generation/utils.py) and the KV-cache reorder that follows the surviving beams (`_reorder_cache` / `Cache.reorder_cache`).
//
// beam_topk, for batch item b with nb beams and logits rows r = b*nb + j:
//   score(j, v) = beam_scores[r] + ((x[r][v] - M_r) - log(Z_r)),  M_r = max_v x[r][v],  Z_r = sum_v exp(x[r][v] - M_r)
// (torch.log_softmax's fp32 formula), and the k best of the nb*V pairs, sorted by score descending, equal scores by the lower flat index
// j*V + v first.  The shift is monotone within a row, so only a row's k largest raw logits can be candidates:
//   launch 1 (seg_kernel): one 256-thread workgroup per (row, segment of SEG = 4096 logits): the segment's max, its sum of exp(x - max) and its
//            k largest logits (equal logits: lower index first);
//   launch 2 (merge_kernel): one workgroup per batch item, one wave per beam: the wave folds its row's segments into M_r, Z_r and the row's top
//            k, scores them, and wave 0 picks the item's top k of the nb*k scored candidates.
// Rows that are log-probabilities already (logprobs: avllm_logits_process normalised them and applied HF's processors, which beam search runs on
// log-probabilities) are scored as beam_scores[r] + x[r][v]; the selection is the same, and -inf entries order below every finite one.
// Keys are 64-bit: an order-preserving uint32 image of the float above 0xffffffff - index, so one unsigned max picks the larger value and,
// among equal values, the lower index.  A selection step is k rounds of a wave-wide max over keys held in registers (k <= 32, no LDS sort).
//
// kv_gather_rows: dst[l, r, t, :] = src[l, parent[r], t, :] for K and V.  One workgroup owns one (tensor, layer, position, column chunk) slice
// for ALL destination rows: it loads every row's source slice into LDS, waits at a barrier, and only then stores.  No other workgroup
// reads or writes that slice, so an in-place gather (src == dst) is correct for any parent map (permutations, several rows from one parent, a
// row that is read and overwritten) without scratch memory.  In place, rows with parent[r] == r are neither read nor written.
#include "common.h"
#include "avllm_internal.h"

namespace {

constexpr int SEG = 4096, SEG_NT = 256, SEG_PT = SEG / SEG_NT;    // segment kernel: 16 logits per thread
constexpr int MAX_NB = 16, MAX_K = 32;

__device__ __forceinline__ uint32_t fkey(float x) {
    const uint32_t u = __float_as_uint(x + 0.0f);                   // -0 -> +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ uint64_t mkkey(float x, uint32_t idx) { return ((uint64_t)fkey(x) << 32) | (0xffffffffu - idx); }
__device__ __forceinline__ uint32_t key_idx(uint64_t k) { return 0xffffffffu - (uint32_t)k; }

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint64_t w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The k largest keys held by one wave (PL per lane, 0 = empty), in descending order: lane i < k returns the i-th, the other lanes 0.  Keys
// are unique (they carry an index), so exactly one lane owns each round's maximum.  Fewer than k non-empty keys leave 0 in the tail.
template <int PL>
__device__ __forceinline__ uint64_t wave_topk(uint64_t (&v)[PL], int k) {
    const int lane = threadIdx.x & (AV_WAVE - 1);
    uint64_t best = 0, mine = 0;
#pragma unroll
    for (int i = 0; i < PL; ++i) best = v[i] > best ? v[i] : best;
    for (int r = 0; r < k; ++r) {
        const uint64_t w = wave_max_u64(best);
        if (lane == r) mine = w;
        if (w != 0 && best == w) {
            best = 0;
#pragma unroll
            for (int i = 0; i < PL; ++i) {
                if (v[i] == w) v[i] = 0;
                best = v[i] > best ? v[i] : best;
            }
        }
    }
    return mine;
}

// grid (nseg, rows), 256 threads.  seg_keys[(row*nseg + seg)*k + i], seg_stat[(row*nseg + seg)*2 + {0,1}] = {max, sum exp(x - max)}.
__global__ __launch_bounds__(SEG_NT) void seg_kernel(const float* __restrict__ logits, long ld, int V, int k, int nseg,
                                                     uint64_t* __restrict__ seg_keys, float* __restrict__ seg_stat) {
    __shared__ uint64_t wk[SEG_NT / AV_WAVE][MAX_K];
    __shared__ float red[SEG_NT / AV_WAVE];
    const int seg = blockIdx.x, row = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float* g = logits + (long)row * ld;
    const int base = seg * SEG;
    float x[SEG_PT];
    uint64_t kv[SEG_PT];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < SEG_PT; ++i) {
        // wave wv reads the contiguous 1024-logit block [base + wv*1024, +1024): its keys stay in its own registers for the wave top-k
        const int v = base + wv * (SEG / 4) + i * AV_WAVE + lane;
        x[i] = v < V ? g[v] : -INFINITY;
        kv[i] = v < V ? mkkey(x[i], (uint32_t)v) : 0;
        m = fmaxf(m, x[i]);
    }
    m = wave_max_f(m);
    if (lane == 0) red[wv] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < SEG_PT; ++i) s += x[i] > -INFINITY ? expf(x[i] - m) : 0.f;     // an all -inf segment sums to 0, not NaN
    s = wave_sum_f(s);
    if (lane == 0) red[wv] = s;
    const uint64_t top = wave_topk(kv, k);
    if (lane < k) wk[wv][lane] = top;
    __syncthreads();
    const size_t o = (size_t)row * nseg + seg;
    if (wv == 0) {
        // the four waves' k best (k <= 32): lane l takes entry l & 31 of waves (l >> 5) and 2 + (l >> 5)
        uint64_t c[2];
        c[0] = (lane & 31) < k ? wk[lane >> 5][lane & 31] : 0;
        c[1] = (lane & 31) < k ? wk[2 + (lane >> 5)][lane & 31] : 0;
        const uint64_t best = wave_topk(c, k);
        if (lane < k) seg_keys[o * k + lane] = best;
        if (lane == 0) {
            seg_stat[o * 2 + 0] = m;
            seg_stat[o * 2 + 1] = (red[0] + red[1]) + (red[2] + red[3]);
        }
    }
}

// grid B, nb waves.  Wave j: row r = b*nb + j.
__global__ __launch_bounds__(MAX_NB * AV_WAVE) void merge_kernel(const uint64_t* __restrict__ seg_keys, const float* __restrict__ seg_stat,
                                                                 int nb, int V, int k, int nseg, const float* __restrict__ beam_scores,
                                                                 int logprobs, float* __restrict__ out_scores, int32_t* __restrict__ out_beams,
                                                                 int64_t* __restrict__ out_tokens) {
    __shared__ uint64_t cand[MAX_NB * MAX_K];
    const int b = blockIdx.x, lane = threadIdx.x & 63, j = threadIdx.x >> 6, r = b * nb + j;
    const uint64_t* sk = seg_keys + (size_t)r * nseg * k;
    const float* st = seg_stat + (size_t)r * nseg * 2;
    // row statistics: M = max of segment maxima, Z = sum of segment sums rescaled to M
    float M = -INFINITY;
    for (int s = lane; s < nseg; s += AV_WAVE) M = fmaxf(M, st[2 * s]);
    M = wave_max_f(M);
    float Z = 0.f;
    for (int s = lane; s < nseg; s += AV_WAVE) Z += st[2 * s + 1] * expf(st[2 * s] - M);
    Z = wave_sum_f(Z);
    const float lz = logf(Z), bs = beam_scores[r];
    // row top-k: fold the nseg*k segment candidates in chunks of 64*16, carrying the running top-k in one extra slot per lane
    constexpr int PL = 16;
    const int n = nseg * k;
    uint64_t rk = 0;
    for (int c0 = 0; c0 < n; c0 += AV_WAVE * PL) {
        uint64_t c[PL + 1];
#pragma unroll
        for (int i = 0; i < PL; ++i) {
            const int q = c0 + i * AV_WAVE + lane;
            c[i] = q < n ? sk[q] : 0;
        }
        c[PL] = rk;
        rk = wave_topk(c, k);
    }
    // score the row's candidates: key = (score, flat index j*V + v)
    if (lane < k) {
        uint64_t sc = 0;
        if (rk != 0) {
            const float x = unkey((uint32_t)(rk >> 32));
            const float lp = logprobs ? x : (x - M) - lz;
            sc = mkkey(bs + lp, (uint32_t)j * (uint32_t)V + key_idx(rk));
        }
        cand[j * k + lane] = sc;
    }
    __syncthreads();
    if (j == 0) {
        constexpr int CL = MAX_NB * MAX_K / AV_WAVE;              // 8
        uint64_t c[CL];
#pragma unroll
        for (int i = 0; i < CL; ++i) {
            const int q = i * AV_WAVE + lane;
            c[i] = q < nb * k ? cand[q] : 0;
        }
        const uint64_t f = wave_topk(c, k);
        if (lane < k) {
            const uint32_t flat = key_idx(f);
            out_scores[(size_t)b * k + lane] = f ? unkey((uint32_t)(f >> 32)) : -INFINITY;
            out_beams[(size_t)b * k + lane] = f ? (int32_t)(flat / (uint32_t)V) : 0;
            out_tokens[(size_t)b * k + lane] = f ? (int64_t)(flat % (uint32_t)V) : 0;
        }
    }
}

// ---------------------------------------------------------------- KV row gather
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int G_NT = 256, G_PER = 8;                                 // up to 2048 vectors (8 per thread) staged per workgroup

template <typename VT>
__global__ __launch_bounds__(G_NT) void gather_kernel(const char* __restrict__ ks, const char* __restrict__ vs, char* kd, char* vd,
                                                      const int32_t* __restrict__ parent, int layers, int rows, int src_rows, long src_T,
                                                      long dst_T, int t0, int nt, int row_vecs, int cvec, int nchunk, bool in_place) {
    // blockIdx.x = ((tensor * layers + l) * nt + t) * nchunk + chunk
    long id = blockIdx.x;
    const int chunk = (int)(id % nchunk); id /= nchunk;
    const int t = t0 + (int)(id % nt); id /= nt;
    const int l = (int)(id % layers);
    const int tensor = (int)(id / layers);
    const VT* src = (const VT*)(tensor ? vs : ks);
    VT* dst = (VT*)(tensor ? vd : kd);
    const int c0 = chunk * cvec, cw = min(cvec, row_vecs - c0), items = rows * cw;
    const VT* sb = src + ((long)l * src_rows * src_T + t) * row_vecs + c0;      // row p of the slice at sb + p * src_T * row_vecs
    VT* db = dst + ((long)l * rows * dst_T + t) * row_vecs + c0;
    const long ss = src_T * row_vecs, ds = dst_T * row_vecs;
    __shared__ VT buf[G_NT * G_PER];                                 // the slice, staged: 32 KB at 16 bytes per vector
    for (int it = threadIdx.x; it < items; it += G_NT) {
        const int r = it / cw, c = it - r * cw, p = parent[r];
        if (p >= 0 && p < src_rows && !(in_place && p == r)) buf[it] = sb[p * ss + c];
    }
    __syncthreads();                                                 // in place: every read of this slice before any write to it
    for (int it = threadIdx.x; it < items; it += G_NT) {
        const int r = it / cw, c = it - r * cw, p = parent[r];
        if (p >= 0 && p < src_rows && !(in_place && p == r)) db[r * ds + c] = buf[it];
    }
}

template <typename VT>
int gather_launch(const void* ks, const void* vs, void* kd, void* vd, const int32_t* parent, int layers, int rows, int src_rows, long src_T,
                  long dst_T, int t0, int t1, long row_bytes, hipStream_t st) {
    const int row_vecs = (int)(row_bytes / sizeof(VT));
    int cvec = (G_NT * G_PER) / rows;
    if (cvec > row_vecs) cvec = row_vecs;
    const int nchunk = (row_vecs + cvec - 1) / cvec, nt = t1 - t0;
    const long grid = 2L * layers * nt * nchunk;
    AV_CHECK_ARG(grid < (1L << 31), "kv_gather_rows: grid too large");
    hipLaunchKernelGGL(gather_kernel<VT>, dim3((unsigned)grid), dim3(G_NT), 0, st, (const char*)ks, (const char*)vs, (char*)kd, (char*)vd,
                       parent, layers, rows, src_rows, src_T, dst_T, t0, nt, row_vecs, cvec, nchunk, ks == kd);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // namespace

size_t av_beam_topk_workspace_bytes(long rows, int V, int k) {
    const long nseg = (V + SEG - 1) / SEG;
    return (size_t)rows * nseg * ((size_t)k * 8 + 8);
}

int av_beam_topk(const float* logits, long ld, int B, int nb, int V, const float* beam_scores, int k, float* out_scores, int32_t* out_beams,
                 int64_t* out_tokens, void* ws, size_t ws_bytes, int logprobs, hipStream_t st) {
    AV_CHECK_ARG(logits && beam_scores && out_scores && out_beams && out_tokens && ws, "beam_topk: null pointer");
    AV_CHECK_ARG(B > 0 && V > 0 && ld >= V, "beam_topk: bad shape (B %d, V %d, ld %ld)", B, V, ld);
    AV_CHECK_ARG(nb >= 1 && nb <= MAX_NB, "beam_topk: num_beams must be in [1, %d] (got %d)", MAX_NB, nb);
    AV_CHECK_ARG(k >= 1 && k <= MAX_K, "beam_topk: k must be in [1, %d] (got %d)", MAX_K, k);
    AV_CHECK_ARG((long)k <= (long)nb * V, "beam_topk: k = %d > num_beams * V", k);
    AV_CHECK_ARG((unsigned long long)nb * (unsigned long long)V < 0xffffffffull, "beam_topk: num_beams * V must fit 32 bits");
    const long rows = (long)B * nb;
    AV_CHECK_ARG(rows < 65536, "beam_topk: B * num_beams = %ld rows", rows);
    const int nseg = (V + SEG - 1) / SEG;
    const size_t need = av_beam_topk_workspace_bytes(rows, V, k);
    if (ws_bytes < need) return av_set_error(AV_ERR_WORKSPACE, "beam_topk: workspace %zu < %zu bytes", ws_bytes, need);
    uint64_t* seg_keys = (uint64_t*)ws;
    float* seg_stat = (float*)(seg_keys + (size_t)rows * nseg * k);
    hipLaunchKernelGGL(seg_kernel, dim3(nseg, (unsigned)rows), dim3(SEG_NT), 0, st, logits, ld, V, k, nseg, seg_keys, seg_stat);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(merge_kernel, dim3(B), dim3(nb * AV_WAVE), 0, st, seg_keys, seg_stat, nb, V, k, nseg, beam_scores, logprobs, out_scores,
                       out_beams, out_tokens);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_kv_gather_rows(const void* k_src, const void* v_src, int src_rows, long src_T, void* k_dst, void* v_dst, int dst_rows, long dst_T,
                      int layers, int dkv, const int32_t* parent, int t0, int t1, int dtype, hipStream_t st) {
    AV_CHECK_ARG(k_src && v_src && k_dst && v_dst && parent, "kv_gather_rows: null pointer");
    AV_CHECK_ARG(dtype == AV_F32 || dtype == AV_BF16, "kv_gather_rows: dtype");
    AV_CHECK_ARG(layers > 0 && dkv > 0 && src_rows > 0 && dst_rows > 0, "kv_gather_rows: bad shape");
    AV_CHECK_ARG(dst_rows <= G_NT * G_PER, "kv_gather_rows: at most %d destination rows (got %d)", G_NT * G_PER, dst_rows);
    AV_CHECK_ARG(0 <= t0 && t0 <= t1 && t1 <= src_T && t1 <= dst_T, "kv_gather_rows: positions [%d, %d) outside the caches", t0, t1);
    AV_CHECK_ARG((k_src == k_dst) == (v_src == v_dst), "kv_gather_rows: K and V must both be in place or both out of place");
    if (k_src == k_dst) AV_CHECK_ARG(src_rows == dst_rows && src_T == dst_T, "kv_gather_rows: in place needs equal shapes");
    if (t0 == t1) return AV_OK;
    const long row_bytes = (long)dkv * (long)av_dtype_size(dtype);
    const uintptr_t al = (uintptr_t)k_src | (uintptr_t)v_src | (uintptr_t)k_dst | (uintptr_t)v_dst;
    if (row_bytes % 16 == 0 && al % 16 == 0)
        return gather_launch<u32x4>(k_src, v_src, k_dst, v_dst, parent, layers, dst_rows, src_rows, src_T, dst_T, t0, t1, row_bytes, st);
    if (row_bytes % 4 == 0 && al % 4 == 0)
        return gather_launch<uint32_t>(k_src, v_src, k_dst, v_dst, parent, layers, dst_rows, src_rows, src_T, dst_T, t0, t1, row_bytes, st);
    return gather_launch<uint16_t>(k_src, v_src, k_dst, v_dst, parent, layers, dst_rows, src_rows, src_T, dst_T, t0, t1, row_bytes, st);
}
