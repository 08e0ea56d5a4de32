// Single-token attention of the fused token step (decode.hip), over the KV cache in either of its forms.  ONE pass: a group of G = hd/N lanes
// owns cache rows t = g, g + R, ... and carries a running (max, sum, weighted V) triple; the K and V rows of a trip (UN = 4 passes of the
// workgroup) are all requested before the first is used.  Groups are merged through shuffles (same wave) and LDS (NW waves).  No score buffer:
// Tk is unbounded and may come from device memory.  fp32 throughout.
//
// There is one kernel; what a cache form decides is its row form and nothing else:
//   PlainRow<T>  bf16 or float rows [B, Tmax, Hkv hd]: a lane owns N = 8 elements of a row
//   E4m3Row      the block-scaled image of kv_fp8.hip: a lane owns N = 16 codes of a row (one 16-byte load + the block's exponent byte), so a
//                pass covers twice the rows of the bf16 form and a trip keeps the same bytes per lane in flight (4 x 32 code bytes; 128 KiB per
//                1024-thread workgroup).  Dequantisation is exact: code x 2^e, the power of two applied once to the lane's partial score and
//                once to the softmax weight.
// A row form supplies N, the q / output element type Elem, the cache arguments Cache, what a lane holds in flight of one K or one V row (Raw),
// zero(k, v), load(t, k, v), dot(qv, k) (the lane's partial score) and values(v, vf) (the lane's V elements in fp32; returns the factor the
// softmax weight takes).  The K and V rows in flight are two arrays of Raw and the weighted sum over vf is written in the kernel, not in the
// form: with K and V of a row in one struct, or with the accumulators handed to a form's function, the compiler leaves some of the 16-wave
// kernels' multiply-adds unfused that it fuses here (v_pk_mul + v_pk_add for v_pk_fma), which changes the last bit of the sums.
#include "common.h"
#include "avllm_internal.h"
#include "mx.h"

namespace {

#include "attention_decode_rows.h"      // PlainRow<T>, E4m3Row: shared with attention_decode_shared.hip

template <class Row, int NW>
__global__ __launch_bounds__(NW * 64) void attn_decode1_kernel(const typename Row::Elem* __restrict__ q, long ldq, const typename Row::Cache cache,
                                                               typename Row::Elem* __restrict__ o, long ldo, int H, int hd, int Tk,
                                                               const int* __restrict__ tk_dev, int Tmax, float scale, int GQ) {
    constexpr int N = Row::N;
    __shared__ float pacc[NW][128];
    __shared__ float pm[NW], pl[NW];
    const int h = blockIdx.x, b = blockIdx.y, d = (H / GQ) * hd;
    if (tk_dev) Tk += *tk_dev;
    Tk = Tk > Tmax ? Tmax : Tk;                      // a device-side length the host could not check never reads past the cache
    const int G = hd >> __builtin_ctz(N), R = NW * 64 / G;
    const int tid = threadIdx.x, dc = tid % G, rsub = tid / G;
    float qv[N];
    load_f<N>(q + (long)b * ldq + (long)h * hd + dc * N, qv);
#pragma unroll
    for (int j = 0; j < N; ++j) qv[j] *= scale;
    const Row row(cache, b, Tmax, d, h / GQ, hd, dc);
    constexpr int UN = 4;
    float mx = -INFINITY, l = 0.f, acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.f;
    for (int t0 = 0; t0 < Tk; t0 += UN * R) {
        typename Row::Raw kr[UN], vr[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int t = t0 + u * R + rsub;
            Row::zero(kr[u], vr[u]);
            if (t < Tk) row.load(t, kr[u], vr[u]);
        }
        float s[UN], tm = mx;
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int t = t0 + u * R + rsub;
            float x = Row::dot(qv, kr[u]);
            for (int off = G >> 1; off > 0; off >>= 1) x += __shfl_xor(x, off);
            s[u] = t < Tk ? x : -INFINITY;
            tm = fmaxf(tm, s[u]);
        }
        if (tm > -INFINITY) {
            const float f = __expf(mx - tm);             // mx = -inf on the first trip: exp(-inf) = 0, acc and l are 0 anyway
            l *= f;
#pragma unroll
            for (int j = 0; j < N; ++j) acc[j] *= f;
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const float p = __expf(s[u] - tm);       // -inf rows: 0
                l += p;
                float vf[N];
                const float pv = p * Row::values(vr[u], vf);
#pragma unroll
                for (int j = 0; j < N; ++j) acc[j] += pv * vf[j];
            }
            mx = tm;
        }
    }
    // merge the row groups of a wave (lanes with equal dc)
    for (int off = G; off < 64; off <<= 1) {
        const float m2 = __shfl_xor(mx, off), l2 = __shfl_xor(l, off);
        const float mn = fmaxf(mx, m2);
        const float f1 = mx > -INFINITY ? __expf(mx - mn) : 0.f, f2 = m2 > -INFINITY ? __expf(m2 - mn) : 0.f;
        l = l * f1 + l2 * f2;
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = acc[j] * f1 + __shfl_xor(acc[j], off) * f2;
        mx = mn;
    }
    const int w = tid >> 6, lane = tid & 63;
    if (lane < G) {
#pragma unroll
        for (int j = 0; j < N; ++j) pacc[w][lane * N + j] = acc[j];
        if (lane == 0) { pm[w] = mx; pl[w] = l; }
    }
    __syncthreads();
    if (tid < hd) {
        float mn = -INFINITY;
#pragma unroll
        for (int x = 0; x < NW; ++x) mn = fmaxf(mn, pm[x]);
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int x = 0; x < NW; ++x) {
            const float f = pm[x] > -INFINITY ? __expf(pm[x] - mn) : 0.f;
            num += pacc[x][tid] * f;
            den += pl[x] * f;
        }
        o[(long)b * ldo + (long)h * hd + tid] = from_f<typename Row::Elem>(num / den);
    }
}

template <class Row>
int launch_decode1(const void* q, long ldq, typename Row::Cache c, void* o, long ldo, int B, int H, int hd, int Tk, const int* tk_dev, int Tmax, float scale,
                   int G, hipStream_t st) {
    typedef typename Row::Elem T;
    const dim3 grid(H, B);
    // few (sequence, head) pairs: 16 waves each so that a CU still has ~64 KiB of cache rows in flight
    if ((long)B * H <= 1024) hipLaunchKernelGGL((attn_decode1_kernel<Row, 16>), grid, dim3(1024), 0, st, (const T*)q, ldq, c, (T*)o, ldo, H, hd, Tk, tk_dev, Tmax, scale, G);
    else hipLaunchKernelGGL((attn_decode1_kernel<Row, 4>), grid, dim3(256), 0, st, (const T*)q, ldq, c, (T*)o, ldo, H, hd, Tk, tk_dev, Tmax, scale, G);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int av_attention_decode1(const void* q, long ldq, const void* kc, const void* vc, void* o, long ldo, int B, int H, int hd, int Tk, const int* tk_dev,
                         int Tmax, float scale, int dtype, hipStream_t st, int G) {
    AV_CHECK_ARG(q && kc && vc && o && (tk_dev || (Tk > 0 && Tk <= Tmax)) && G > 0 && H % G == 0, "attention_decode: bad args");
    AV_CHECK_ARG((hd == 64 || hd == 128) && ldq % 8 == 0, "attention_decode: head_dim %d unsupported", hd);
    if (dtype == AV_F32) return launch_decode1<PlainRow<float>>(q, ldq, {(const float*)kc, (const float*)vc}, o, ldo, B, H, hd, Tk, tk_dev, Tmax, scale, G, st);
    return launch_decode1<PlainRow<bf16>>(q, ldq, {(const bf16*)kc, (const bf16*)vc}, o, ldo, B, H, hd, Tk, tk_dev, Tmax, scale, G, st);
}

int av_attention_decode_kv8(const void* q, long ldq, const void* kq, const void* ke, const void* vq, const void* ve, void* o, long ldo, int B, int H, int hd,
                            int Tk, const int* tk_dev, int Tmax, float scale, int G, hipStream_t st) {
    AV_CHECK_ARG(q && kq && ke && vq && ve && o && B > 0 && H > 0 && Tmax > 0 && (tk_dev || (Tk > 0 && Tk <= Tmax)) && G > 0 && H % G == 0,
                 "attention_decode_kv8: bad args");
    AV_CHECK_ARG((hd == 64 || hd == 128) && ldq % 8 == 0 && al16(q) && al16(kq) && al16(vq), "attention_decode_kv8: head_dim %d unsupported (64 or 128), q rows and code planes 16-byte aligned", hd);
    return launch_decode1<E4m3Row>(q, ldq, {(const uint8_t*)kq, (const uint8_t*)ke, (const uint8_t*)vq, (const uint8_t*)ve}, o, ldo, B, H, hd, Tk, tk_dev, Tmax,
                                   scale, G, st);
}

extern "C" int avllm_attention_decode(const void* q, int64_t ldq, const void* kc, const void* vc, void* o, int64_t ldo, int32_t B, int32_t H, int32_t hd,
                                      int32_t Tk, const int32_t* tk_dev, int32_t Tmax, float scale, int32_t kv_group, int32_t dtype, void* stream) {
    AV_CHECK_ARG(B > 0 && H > 0 && (dtype == AV_F32 || dtype == AV_BF16), "attention_decode: B=%d H=%d dtype=%d", B, H, dtype);
    return av_attention_decode1(q, ldq, kc, vc, o, ldo, B, H, hd, Tk, tk_dev, Tmax, scale, dtype, (hipStream_t)stream, kv_group);
}
extern "C" int avllm_attention_decode_kv8(const void* q, int64_t ldq, const void* k_codes, const void* k_exps, const void* v_codes, const void* v_exps, void* o,
                                          int64_t ldo, int32_t B, int32_t H, int32_t hd, int32_t Tk, const int32_t* tk_dev, int32_t Tmax, float scale,
                                          int32_t kv_group, void* stream) {
    return av_attention_decode_kv8(q, ldq, k_codes, k_exps, v_codes, v_exps, o, ldo, B, H, hd, Tk, tk_dev, Tmax, scale, kv_group, (hipStream_t)stream);
}
