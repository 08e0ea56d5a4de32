// Single-token attention of the token step when the `group` rows of an item (its beams, or its sampled sequences) share the item's prefix:
// row r of R = B group attends prefix rows [0, S) of item r / group, stored ONCE in the B-row cache the prefill wrote, followed by its own
// suffix rows [0, Tk) of an R-row cache [R, N, Hkv hd].  The result is the softmax over the concatenation, fp32 throughout, as
// attn_decode1_kernel (attention_decode.hip) computes it over an R-row copy of the same keys, up to fp32 summation order.  Two launches:
//
//   attn_shared_prefix_kernel   grid (H, B passes, nsplit): a workgroup streams its slice of the item's prefix for one query head once and
//                               applies every K / V row, held in registers, to QC <= 4 queries of that head (the item's rows; a larger group
//                               is ceil(group / 4) passes, each a workgroup of its own: they run side by side and the slice's second reader
//                               finds it in L2).  One running (max, sum, acc[hd]) per query; one fp32 partial (max, sum, acc[hd]) per (row,
//                               head, slice) goes to the workspace.
//   attn_shared_out_kernel      grid (H, R): the row's own suffix rows, then the nsplit prefix partials of its (row, head) merged in with the
//                               usual max-rescale, one division, the output.
// Where the prefix launch could not fill the chip even with one trip per workgroup (few items and a short prefix: sh_nsplit), the second
// kernel alone runs the whole attention with 16 waves over prefix and suffix as one sequence of keys: one launch, as the copy form has.
//
// The split over the prefix is what keeps the CUs fed: sharing divides the (sequence, head) pairs by `group` (128 at B = 4 on Llama-2-7B for
// 256 CUs), and a workgroup's time is its trips one after the other (a trip = UN = 4 passes, 32 KiB of bf16 rows at hd 128, requested
// before the first is used).  So the prefix is cut into slices (sh_nsplit: as many as fill the chip with ONE round of resident workgroups,
// 16 at the most and never below one trip each; 6 for 4 x 4 rows of a bf16 Llama-2-7B cache).  A pass wholly past the slice's end costs no
// arithmetic, and the suffix launch requests its row's partials before it streams the suffix.
//
// No atomics, and every sum is a fixed sequence of explicit fmaf: identical inputs give identical bits from launch to launch, and a query's
// arithmetic does not depend on the slot of the pass it rides in, so beams with equal q and equal suffix get equal outputs.
// The row forms are attention_decode.hip's (attention_decode_rows.h); the e4m3 form dequantises a K or V row once for all QC queries.
#include "common.h"
#include "avllm_internal.h"
#include "mx.h"

namespace {

#include "attention_decode_rows.h"

constexpr int SH_NW = 4;            // waves per workgroup, both launches
constexpr int SH_UN = 4;            // passes of the workgroup per trip
constexpr int SH_QC = 4;            // most queries per pass of the prefix launch (registers: QC (2 N + 2) per lane besides the rows in flight)
constexpr int SH_MAX_SPLIT = 16;
constexpr int SH_ONE_NW = 16;       // waves of the one-launch form (attn_decode1_kernel's count for few (sequence, head) pairs)

// the prefix rows of an item followed by the suffix rows of one of its rows, as ONE sequence of keys: row t < S is the prefix', t - S the suffix'
template <class Row> struct JoinedRows {
    Row pre, suf; int S;
    __device__ __forceinline__ void load(int t, typename Row::Raw& k, typename Row::Raw& v) const {
        if (t < S) pre.load(t, k, v);
        else suf.load(t - S, k, v);
    }
};

// rows [t_lo, t_hi) of `row` (a Row, or JoinedRows<Row>) applied to QC queries: lane group rsub of RW owns rows t_lo + rsub, + RW, ...; G lanes
// share a row
template <class Row, int QC, class Rows>
__device__ __forceinline__ void sh_stream(const Rows& row, const float (&qv)[QC][Row::N], int t_lo, int t_hi, int rsub, int RW, int G, float (&mx)[QC],
                                          float (&l)[QC], float (&acc)[QC][Row::N]) {
    constexpr int N = Row::N;
    for (int t0 = t_lo; t0 < t_hi; t0 += SH_UN * RW) {
        typename Row::Raw kr[SH_UN], vr[SH_UN];
#pragma unroll
        for (int u = 0; u < SH_UN; ++u) {
            const int t = t0 + u * RW + rsub;
            Row::zero(kr[u], vr[u]);
            if (t < t_hi) row.load(t, kr[u], vr[u]);
        }
        float s[SH_UN][QC], tm[QC];
#pragma unroll
        for (int j = 0; j < QC; ++j) tm[j] = mx[j];
#pragma unroll
        for (int u = 0; u < SH_UN; ++u) {
#pragma unroll
            for (int j = 0; j < QC; ++j) s[u][j] = -INFINITY;
            if (t0 + u * RW >= t_hi) continue;                  // a pass wholly past the slice (the same for every lane): no arithmetic
            const bool live = t0 + u * RW + rsub < t_hi;
            float kf[N];
            const float ks = Row::values(kr[u], kf);
#pragma unroll
            for (int j = 0; j < QC; ++j) {
                float x = 0.f;
#pragma unroll
                for (int e = 0; e < N; ++e) x = __builtin_fmaf(qv[j][e], kf[e], x);
                x *= ks;
                for (int off = G >> 1; off > 0; off >>= 1) x += __shfl_xor(x, off);
                s[u][j] = live ? x : -INFINITY;
                tm[j] = fmaxf(tm[j], s[u][j]);
            }
        }
#pragma unroll
        for (int j = 0; j < QC; ++j) {
            // nothing seen yet (the lane's rows of a last trip are all past t_hi): exponents against 0, every weight is exp(-inf) = 0
            const float te = tm[j] > -INFINITY ? tm[j] : 0.f;
            const float f = __expf(mx[j] - te);
            l[j] *= f;
#pragma unroll
            for (int e = 0; e < N; ++e) acc[j][e] *= f;
            mx[j] = tm[j];
            tm[j] = te;
        }
#pragma unroll
        for (int u = 0; u < SH_UN; ++u) {
            if (t0 + u * RW >= t_hi) continue;
            float vf[N];
            const float vs = Row::values(vr[u], vf);
#pragma unroll
            for (int j = 0; j < QC; ++j) {
                const float p = __expf(s[u][j] - tm[j]);
                l[j] += p;
                const float pv = p * vs;
#pragma unroll
                for (int e = 0; e < N; ++e) acc[j][e] = __builtin_fmaf(pv, vf[e], acc[j][e]);
            }
        }
    }
}

// one query's state merged over the lane groups of a wave (lanes with equal dc); every lane ends with the wave's state
template <int N> __device__ __forceinline__ void sh_merge_wave(float& mx, float& l, float (&acc)[N], int G) {
    for (int off = G; off < 64; off <<= 1) {
        const float m2 = __shfl_xor(mx, off), l2 = __shfl_xor(l, off);
        const float mn = fmaxf(mx, m2);
        const float f1 = mx > -INFINITY ? __expf(mx - mn) : 0.f, f2 = m2 > -INFINITY ? __expf(m2 - mn) : 0.f;
        l = __builtin_fmaf(l, f1, l2 * f2);
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = __builtin_fmaf(acc[j], f1, __shfl_xor(acc[j], off) * f2);
        mx = mn;
    }
}

// part: [R, H, nsplit, 2 + hd] f32 = (max, sum, acc[hd]) of the prefix slice [z per, z per + per) for row r, head h
template <class Row, int QC>
__global__ __launch_bounds__(SH_NW * 64) void attn_shared_prefix_kernel(const typename Row::Elem* __restrict__ q, long ldq, const typename Row::Cache cache,
                                                                        float* __restrict__ part, int H, int hd, int S, int Tp, int group, float scale,
                                                                        int GQ) {
    constexpr int N = Row::N;
    __shared__ float pacc[SH_NW][QC][128];
    __shared__ float pm[SH_NW][QC], pl[SH_NW][QC];
    const int npass = (group + QC - 1) / QC;                           // blockIdx.y = item, pass of QC queries
    const int h = blockIdx.x, b = blockIdx.y / npass, g0 = (blockIdx.y - b * npass) * QC, z = blockIdx.z, nsplit = gridDim.z, d = (H / GQ) * hd;
    const int per = (S + nsplit - 1) / nsplit, t_lo = z * per, t_hi = t_lo + per < S ? t_lo + per : S;      // an empty slice leaves (-inf, 0, 0)
    const int G = hd >> __builtin_ctz(N), RW = SH_NW * 64 / G;
    const int tid = threadIdx.x, dc = tid % G, rsub = tid / G, w = tid >> 6, lane = tid & 63;
    const Row row(cache, b, Tp, d, h / GQ, hd, dc);
    float qv[QC][N], mx[QC], l[QC], acc[QC][N];
#pragma unroll
    for (int j = 0; j < QC; ++j) {
        const int g = g0 + j < group ? g0 + j : group - 1;               // a slot past the group rides along on the last row; nothing of it is written
        load_f<N>(q + (long)(b * group + g) * ldq + (long)h * hd + dc * N, qv[j]);
        mx[j] = -INFINITY;
        l[j] = 0.f;
#pragma unroll
        for (int e = 0; e < N; ++e) { qv[j][e] *= scale; acc[j][e] = 0.f; }
    }
    sh_stream<Row, QC>(row, qv, t_lo, t_hi, rsub, RW, G, mx, l, acc);
#pragma unroll
    for (int j = 0; j < QC; ++j) {
        sh_merge_wave<N>(mx[j], l[j], acc[j], G);
        if (lane < G) {
#pragma unroll
            for (int e = 0; e < N; ++e) pacc[w][j][lane * N + e] = acc[j][e];
            if (lane == 0) { pm[w][j] = mx[j]; pl[w][j] = l[j]; }
        }
    }
    __syncthreads();
    if (tid >= hd) return;
#pragma unroll
    for (int j = 0; j < QC; ++j) {
        if (g0 + j >= group) break;
        float mn = -INFINITY;
#pragma unroll
        for (int x = 0; x < SH_NW; ++x) mn = fmaxf(mn, pm[x][j]);
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int x = 0; x < SH_NW; ++x) {
            const float f = pm[x][j] > -INFINITY ? __expf(pm[x][j] - mn) : 0.f;
            num = __builtin_fmaf(pacc[x][j][tid], f, num);
            den = __builtin_fmaf(pl[x][j], f, den);
        }
        float* o = part + (((long)(b * group + g0 + j) * H + h) * nsplit + z) * (hd + 2);
        if (tid == 0) { o[0] = mn; o[1] = den; }
        o[2 + tid] = num;
    }
}

// The launch that writes the output, grid (H, R), in two forms:
//   ONE = false, 4 waves:   the row's suffix rows, then the nsplit prefix partials of attn_shared_prefix_kernel
//   ONE = true, 16 waves:   the whole attention in this launch, as attn_decode1_kernel runs it over a copy cache: prefix and suffix are one
//                           sequence of S + Tk keys (JoinedRows) and there are no partials.  For shapes whose prefix launch could not fill the
//                           chip (launch_shared): the item's prefix is then read `group` times, mostly from L2, but stored once all the same.
template <class Row, int NW, bool ONE>
__global__ __launch_bounds__(NW * 64) void attn_shared_out_kernel(const typename Row::Elem* __restrict__ q, long ldq, const typename Row::Cache pre, int S, int Tp,
                                                                  int group, const typename Row::Cache cache, const float* __restrict__ part, int nsplit,
                                                                  typename Row::Elem* __restrict__ o, long ldo, int H, int hd, int Tk,
                                                                  const int* __restrict__ tk_dev, int Tmax, float scale, int GQ) {
    constexpr int N = Row::N;
    __shared__ float pacc[NW][128];
    __shared__ float pm[NW], pl[NW];
    const int h = blockIdx.x, r = blockIdx.y, d = (H / GQ) * hd;
    if (tk_dev) Tk += *tk_dev;
    Tk = Tk > Tmax ? Tmax : Tk;                      // a device-side length the host could not check never reads past the suffix cache
    Tk = Tk < 0 ? 0 : Tk;
    const int G = hd >> __builtin_ctz(N), RW = NW * 64 / G;
    const int tid = threadIdx.x, dc = tid % G, rsub = tid / G, w = tid >> 6, lane = tid & 63;
    // the prefix partials of this (row, head), requested before the suffix is streamed: read one after the other at the end, every slice
    // would cost a trip to memory of its own
    constexpr int NZ = ONE ? 1 : SH_MAX_SPLIT;
    float zm[NZ], zl[NZ], za[NZ];
#pragma unroll
    for (int z = 0; z < NZ; ++z) {
        const bool on = !ONE && z < nsplit && tid < hd;
        const float* pz = part + (((long)r * H + h) * nsplit + (on ? z : 0)) * (hd + 2);
        zm[z] = on ? pz[0] : -INFINITY;
        zl[z] = on ? pz[1] : 0.f;
        za[z] = on ? pz[2 + tid] : 0.f;
    }
    float qv[1][N], mx[1] = {-INFINITY}, l[1] = {0.f}, acc[1][N];
    load_f<N>(q + (long)r * ldq + (long)h * hd + dc * N, qv[0]);
#pragma unroll
    for (int e = 0; e < N; ++e) { qv[0][e] *= scale; acc[0][e] = 0.f; }
    const Row row(cache, r, Tmax, d, h / GQ, hd, dc);
    if constexpr (ONE) {
        const JoinedRows<Row> both = {Row(pre, r / group, Tp, d, h / GQ, hd, dc), row, S};
        sh_stream<Row, 1>(both, qv, 0, S + Tk, rsub, RW, G, mx, l, acc);
    } else {
        sh_stream<Row, 1>(row, qv, 0, Tk, rsub, RW, G, mx, l, acc);
    }
    sh_merge_wave<N>(mx[0], l[0], acc[0], G);
    if (lane < G) {
#pragma unroll
        for (int e = 0; e < N; ++e) pacc[w][lane * N + e] = acc[0][e];
        if (lane == 0) { pm[w] = mx[0]; pl[w] = l[0]; }
    }
    __syncthreads();
    if (tid < hd) {
        float mn = -INFINITY;
#pragma unroll
        for (int x = 0; x < NW; ++x) mn = fmaxf(mn, pm[x]);
#pragma unroll
        for (int z = 0; z < NZ; ++z) mn = fmaxf(mn, zm[z]);
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int z = 0; z < NZ; ++z) {               // the prefix first, in slice order (slices past nsplit: weight 0), then this launch's waves
            const float f = zm[z] > -INFINITY ? __expf(zm[z] - mn) : 0.f;
            num = __builtin_fmaf(za[z], f, num);
            den = __builtin_fmaf(zl[z], f, den);
        }
#pragma unroll
        for (int x = 0; x < NW; ++x) {
            const float f = pm[x] > -INFINITY ? __expf(pm[x] - mn) : 0.f;
            num = __builtin_fmaf(pacc[x][tid], f, num);
            den = __builtin_fmaf(pl[x], f, den);
        }
        o[(long)r * ldo + (long)h * hd + tid] = from_f<typename Row::Elem>(num / den);
    }
}

// Slices of the prefix for wg = H B passes workgroups per slice; 0 = no prefix launch, the one-launch form.
// Two launches: ONE round of resident workgroups, at most 16 slices and never less than one trip each.  At Llama-2-7B shapes (2 .. 16 slices
// forced: profiles/r17_beam_shared_prefix_bench.txt) the launch is fastest where its workgroups just fill the chip once -- 6 slices for 4 x 4 rows
// of a bf16 cache (3 workgroups per CU by registers), 4 for the e4m3 image (2 per CU) -- and a third of a round more costs a whole one.
// One launch: where the prefix has fewer trips than the chip holds workgroups (wg trips < resident: one item of 4 beams at 544 positions, 16 rows
// at 256), even one trip per workgroup leaves CUs idle and two launches cost more than the copy form's one.
// Knob SHARED_SPLIT (A/B runs and tests): n > 0 forces n slices, -1 the one-launch form.
// The occupancy is asked once per kernel, at its first launch: a caller that captures the step into a graph runs it once before (as every
// capture here does, to size workspaces).
template <class Row, int QC> int sh_nsplit(int wg, int hd, int S) {
    const int forced = av_knob(AV_KNOB_SHARED_SPLIT);
    if (forced) return forced < 0 ? 0 : forced < SH_MAX_SPLIT ? forced : SH_MAX_SPLIT;
    static const int per_cu = [] {                              // workgroups of this kernel a CU holds at a time
        int v = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, attn_shared_prefix_kernel<Row, QC>, SH_NW * 64, 0) == hipSuccess && v > 0 ? v : 2;
    }();
    int ncu = 256;
    av_device(&ncu);
    const int trip = SH_UN * (SH_NW * 64 / (hd / Row::N)), trips = (S + trip - 1) / trip;
    if ((long)wg * trips < (long)ncu * per_cu) return 0;
    int n = ncu * per_cu / wg;
    n = n < trips ? n : trips;
    n = n < SH_MAX_SPLIT ? n : SH_MAX_SPLIT;
    return n < 1 ? 1 : n;
}

template <class Row, int QC>
int launch_prefix(const typename Row::Elem* q, long ldq, typename Row::Cache pre, float* part, int B, int group, int H, int hd, int S, int Tp, float scale, int GQ,
                  hipStream_t st, int& nsplit) {
    const int by = B * ((group + QC - 1) / QC);
    nsplit = sh_nsplit<Row, QC>(H * by, hd, S);
    if (!nsplit) return AV_OK;
    hipLaunchKernelGGL((attn_shared_prefix_kernel<Row, QC>), dim3(H, by, nsplit), dim3(SH_NW * 64), 0, st, q, ldq, pre, part, H, hd, S, Tp, group, scale, GQ);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

template <class Row>
int launch_shared(const void* q, long ldq, typename Row::Cache pre, int S, int Tp, typename Row::Cache suf, int Tk, const int* tk_dev, int N, void* o, long ldo,
                  int R, int group, int H, int hd, float scale, int GQ, void* ws, hipStream_t st) {
    typedef typename Row::Elem T;
    const int B = R / group;
    float* part = (float*)ws;
    int nsplit = 0;
    if (group == 1) AV_TRY((launch_prefix<Row, 1>((const T*)q, ldq, pre, part, B, group, H, hd, S, Tp, scale, GQ, st, nsplit)));
    else if (group == 2) AV_TRY((launch_prefix<Row, 2>((const T*)q, ldq, pre, part, B, group, H, hd, S, Tp, scale, GQ, st, nsplit)));
    else AV_TRY((launch_prefix<Row, SH_QC>((const T*)q, ldq, pre, part, B, group, H, hd, S, Tp, scale, GQ, st, nsplit)));
    if (nsplit) hipLaunchKernelGGL((attn_shared_out_kernel<Row, SH_NW, false>), dim3(H, R), dim3(SH_NW * 64), 0, st, (const T*)q, ldq, pre, S, Tp, group, suf, part,
                                   nsplit, (T*)o, ldo, H, hd, Tk, tk_dev, N, scale, GQ);
    else hipLaunchKernelGGL((attn_shared_out_kernel<Row, SH_ONE_NW, true>), dim3(H, R), dim3(SH_ONE_NW * 64), 0, st, (const T*)q, ldq, pre, S, Tp, group, suf, part,
                            1, (T*)o, ldo, H, hd, Tk, tk_dev, N, scale, GQ);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_shared(const char* who, const void* q, long ldq, const void* o, int S, int Tp, int Tk, const int* tk_dev, int N, int R, int group, int H, int hd,
                 int GQ, const void* ws, size_t ws_bytes) {
    AV_CHECK_ARG(q && o, "%s: q or o is null", who);
    AV_CHECK_ARG(R > 0 && group > 0 && R % group == 0, "%s: R=%d rows must be whole groups of group=%d", who, R, group);
    AV_CHECK_ARG(H > 0 && GQ > 0 && H % GQ == 0, "%s: H=%d heads must be whole kv groups of kv_group=%d", who, H, GQ);
    AV_CHECK_ARG((hd == 64 || hd == 128) && ldq % 8 == 0, "%s: head_dim %d unsupported (64 or 128), q rows 16-byte aligned", who, hd);
    AV_CHECK_ARG(S > 0 && S <= Tp, "%s: S=%d prefix rows outside the prefix cache (Tprefix=%d)", who, S, Tp);
    AV_CHECK_ARG(N > 0 && (tk_dev || (Tk > 0 && Tk <= N)), "%s: Tk=%d suffix rows outside the suffix cache (N=%d)", who, Tk, N);
    AV_CHECK_ARG(ws && ws_bytes >= av_attention_decode_shared_ws(R, H, hd), "%s: ws of %zu bytes, needs %zu (avllm_attention_decode_shared_workspace_bytes)", who,
                 ws_bytes, av_attention_decode_shared_ws(R, H, hd));
    return AV_OK;
}

}  // namespace

size_t av_attention_decode_shared_ws(int R, int H, int hd) {
    return R > 0 && H > 0 && hd > 0 ? (size_t)R * H * SH_MAX_SPLIT * (hd + 2) * sizeof(float) : 0;
}

int av_attention_decode_shared(const void* q, long ldq, const void* kp, const void* vp, int S, int Tp, const void* ks, const void* vs, int Tk, const int* tk_dev,
                               int N, void* o, long ldo, int R, int group, int H, int hd, float scale, int GQ, void* ws, size_t ws_bytes, hipStream_t st) {
    AV_TRY(check_shared("attention_decode_shared", q, ldq, o, S, Tp, Tk, tk_dev, N, R, group, H, hd, GQ, ws, ws_bytes));
    AV_CHECK_ARG(kp && vp, "attention_decode_shared: k_prefix or v_prefix is null");
    AV_CHECK_ARG(ks && vs, "attention_decode_shared: k_suffix or v_suffix is null");
    AV_CHECK_ARG(al16(q) && al16(kp) && al16(vp) && al16(ks) && al16(vs), "attention_decode_shared: q, k_prefix, v_prefix, k_suffix, v_suffix must be 16-byte aligned");
    typedef PlainRow<bf16> Row;
    return launch_shared<Row>(q, ldq, {(const bf16*)kp, (const bf16*)vp}, S, Tp, {(const bf16*)ks, (const bf16*)vs}, Tk, tk_dev, N, o, ldo, R, group, H, hd, scale,
                              GQ, ws, st);
}

int av_attention_decode_shared_kv8(const void* q, long ldq, const void* kpq, const void* kpe, const void* vpq, const void* vpe, int S, int Tp, const void* ksq,
                                   const void* kse, const void* vsq, const void* vse, int Tk, const int* tk_dev, int N, void* o, long ldo, int R, int group, int H,
                                   int hd, float scale, int GQ, void* ws, size_t ws_bytes, hipStream_t st) {
    AV_TRY(check_shared("attention_decode_shared_kv8", q, ldq, o, S, Tp, Tk, tk_dev, N, R, group, H, hd, GQ, ws, ws_bytes));
    AV_CHECK_ARG(kpq && kpe && vpq && vpe && al16(kpq) && al16(vpq), "attention_decode_shared_kv8: k_prefix / v_prefix planes null or codes not 16-byte aligned");
    AV_CHECK_ARG(ksq && kse && vsq && vse && al16(ksq) && al16(vsq), "attention_decode_shared_kv8: k_suffix / v_suffix planes null or codes not 16-byte aligned");
    AV_CHECK_ARG(al16(q), "attention_decode_shared_kv8: q not 16-byte aligned");
    typedef const uint8_t* P;
    return launch_shared<E4m3Row>(q, ldq, {(P)kpq, (P)kpe, (P)vpq, (P)vpe}, S, Tp, {(P)ksq, (P)kse, (P)vsq, (P)vse}, Tk, tk_dev, N, o, ldo, R, group, H, hd, scale,
                                  GQ, ws, st);
}

extern "C" size_t avllm_attention_decode_shared_workspace_bytes(int32_t R, int32_t H, int32_t hd) { return av_attention_decode_shared_ws(R, H, hd); }

extern "C" int avllm_attention_decode_shared(const void* q, int64_t ldq, const void* k_prefix, const void* v_prefix, int32_t S, int32_t Tprefix,
                                             const void* k_suffix, const void* v_suffix, int32_t Tk, const int32_t* tk_dev, int32_t N, void* o, int64_t ldo,
                                             int32_t R, int32_t group, int32_t H, int32_t hd, float scale, int32_t kv_group, void* ws, size_t ws_bytes,
                                             void* stream) {
    return av_attention_decode_shared(q, ldq, k_prefix, v_prefix, S, Tprefix, k_suffix, v_suffix, Tk, tk_dev, N, o, ldo, R, group, H, hd, scale, kv_group, ws,
                                      ws_bytes, (hipStream_t)stream);
}
extern "C" int avllm_attention_decode_shared_kv8(const void* q, int64_t ldq, const void* kp_codes, const void* kp_exps, const void* vp_codes, const void* vp_exps,
                                                 int32_t S, int32_t Tprefix, const void* ks_codes, const void* ks_exps, const void* vs_codes, const void* vs_exps,
                                                 int32_t Tk, const int32_t* tk_dev, int32_t N, void* o, int64_t ldo, int32_t R, int32_t group, int32_t H,
                                                 int32_t hd, float scale, int32_t kv_group, void* ws, size_t ws_bytes, void* stream) {
    return av_attention_decode_shared_kv8(q, ldq, kp_codes, kp_exps, vp_codes, vp_exps, S, Tprefix, ks_codes, ks_exps, vs_codes, vs_exps, Tk, tk_dev, N, o, ldo, R,
                                          group, H, hd, scale, kv_group, ws, ws_bytes, (hipStream_t)stream);
}
