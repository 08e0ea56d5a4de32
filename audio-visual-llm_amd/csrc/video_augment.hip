// Visual augmentation on the device (include/avllm.h, "visual augmentation"): avllm_clip_preproc_aug is avllm_clip_preproc with one random crop
// window, one horizontal flip and masked spans of frames per clip folded into its two passes; avllm_video_frames_augment flips and masks
// pixel_values that were resized and cropped before.  The rule is stated in full in the header and restated on the host by
// tests/refs_video_augment.py.  Nothing on the default path comes here.
#include "common.h"
#include "avllm_internal.h"
#include "resize_coeffs.h"
#include <array>
#include <cstring>
#include <map>
#include <math.h>
#include <mutex>
#include <vector>

namespace {

using namespace av_resize;

constexpr int VA_THREADS = 256;
constexpr int VA_MAX_MASKS = 16;
constexpr int VA_MAX_BLOCKS = 2048;             // the in-place pass is memory-bound: a few blocks per CU, the rest by grid stride
constexpr uint32_t VIDEO_SALT = 0x76696465u;    // "vide"

struct AugHdr {
    int H, W, resize, image, newH, newW, ksx, ksy;
    int off_bx, off_kx, off_by, off_ky, off_lut;          // byte offsets into the plan; bounds and coefficients of ALL newW columns / newH rows
};

struct AugArgs {                                // what the draw of a clip depends on, by value in every launch
    int N, clip, random_crop, n_time, max_tw;
    float ratio;
    uint32_t thr, seed;
    const uint32_t* seed_dev;
};

struct ClipDraw {                               // one per block, in LDS
    int left, top, flip, ylo, yhi;
    int span[VA_MAX_MASKS][2];
};

// clip8 for a byte that is packed into a dword beside others.  Left to itself the code generator folds two neighbouring clamps into one
// v_ashr_pk_u8_i32 and ORs its result into the dword as if the upper half of the destination were zero; on gfx950 that half keeps what the
// register held before (here the last coefficient loaded, all ones when it is negative), which turned the two bytes above it into 255.  The
// empty asm keeps each clamp on its own v_med3_i32.
__device__ __forceinline__ unsigned clip8_lone(int v) {
    int r = clip8(v);
    asm volatile("" : "+v"(r));
    return (unsigned)r;
}

// The draw of clip a.clip with N frames (the header's rule): threads 0 .. n_time-1 take one span each, thread 0 also crop and flip.  Ends in a
// barrier: every thread of the block may read d afterwards.  range_w / range_h = newW - image + 1 / newH - image + 1 (1: no crop to draw).
__device__ __forceinline__ void clip_draw(ClipDraw& d, const AugArgs& a, int N, unsigned long long clip, int range_w, int range_h) {
    const uint32_t s = av_seed(a.seed_dev, a.seed) + VIDEO_SALT;
    const unsigned long long k = 64ull * clip;
    const int j = threadIdx.x;
    if (j < a.n_time) {
        const double cap = floor((double)a.ratio * (double)N);
        const int wmax = (double)a.max_tw < cap ? a.max_tw : (int)cap;
        const uint32_t h = av_pair_hash(s, k + 4 + 2 * j), h2 = av_pair_hash(s, k + 5 + 2 * j);
        const int w = (int)(((unsigned long long)h * (unsigned long long)(wmax + 1)) >> 32);
        d.span[j][0] = (int)(((unsigned long long)h2 * (unsigned long long)(N - w + 1)) >> 32);
        d.span[j][1] = w;
    }
    if (j == 0) {
        d.left = a.random_crop ? (int)(((unsigned long long)av_pair_hash(s, k) * (unsigned long long)range_w) >> 32) : (range_w - 1) / 2;
        d.top = a.random_crop ? (int)(((unsigned long long)av_pair_hash(s, k + 1) * (unsigned long long)range_h) >> 32) : (range_h - 1) / 2;
        d.flip = (av_pair_hash(s, k + 2) >> 8) < a.thr ? 1 : 0;
    }
    __syncthreads();
}

__device__ __forceinline__ bool frame_masked(const ClipDraw& d, int n_time, int n) {
    bool m = false;
    for (int j = 0; j < n_time; ++j) m |= n >= d.span[j][0] && n < d.span[j][0] + d.span[j][1];
    return m;
}

// the fused call's draw plus the input rows [ylo, yhi) that the vertical taps of output rows top .. top + image - 1 reach
__device__ __forceinline__ void fused_draw(ClipDraw& d, const AugHdr* h, const int* by, const AugArgs& a) {
    clip_draw(d, a, a.N, (unsigned long long)a.clip, h->newW - h->image + 1, h->newH - h->image + 1);
    if (threadIdx.x == 0) {
        d.ylo = by[2 * d.top];
        d.yhi = by[2 * (d.top + h->image - 1)] + by[2 * (d.top + h->image - 1) + 1];
    }
    __syncthreads();
}

// horizontal pass, scalar: block (x, n) takes 256 of the H * image cells of frame n's tmp image; a cell of a row outside [ylo, yhi), or of a
// masked frame, is not produced.  tmp [N, H, image, 3] u8 holds column left + xo of the resize at xo (image - 1 - xo when the clip flips).
__global__ __launch_bounds__(VA_THREADS) void aug_resize_h_kernel(const char* __restrict__ plan, const unsigned char* __restrict__ in,
                                                                  unsigned char* __restrict__ tmp, AugArgs a) {
    __shared__ ClipDraw d;
    const AugHdr* h = (const AugHdr*)plan;
    const int* bx = (const int*)(plan + h->off_bx);
    const int* kx = (const int*)(plan + h->off_kx);
    fused_draw(d, h, (const int*)(plan + h->off_by), a);
    const int n = blockIdx.y, S = h->image;
    if (frame_masked(d, a.n_time, n)) return;
    const int i = blockIdx.x * VA_THREADS + threadIdx.x;
    if (i >= h->H * S) return;
    const int y = i / S, xo = i - y * S;
    if (y < d.ylo || y >= d.yhi) return;
    const int c = d.left + (d.flip ? S - 1 - xo : xo);
    const int x0 = bx[2 * c], cnt = bx[2 * c + 1];
    const int* k = kx + (long)c * h->ksx;
    const long row = (long)n * h->H + y;
    const unsigned char* p = in + (row * h->W + x0) * 3;
    int s0 = 1 << (PBITS - 1), s1 = s0, s2 = s0;
    for (int j = 0; j < cnt; ++j) {
        const int cf = k[j];
        s0 += p[3 * j] * cf; s1 += p[3 * j + 1] * cf; s2 += p[3 * j + 2] * cf;
    }
    unsigned char* o = tmp + (row * S + xo) * 3;
    o[0] = (unsigned char)clip8(s0); o[1] = (unsigned char)clip8(s1); o[2] = (unsigned char)clip8(s2);
}

// horizontal pass, staged: block (x, n) copies input rows ylo + x rpb .. of frame n (contiguous bytes) into LDS with aligned dword loads, then
// each thread produces 4 adjacent tmp pixels (12 bytes, three dword stores) from LDS bytes.  Needs image % 4 == 0.
__global__ __launch_bounds__(VA_THREADS) void aug_resize_h4_kernel(const char* __restrict__ plan, const unsigned char* __restrict__ in,
                                                                   unsigned char* __restrict__ tmp, long in_bytes, int rpb, AugArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rows_s[];
    __shared__ ClipDraw d;
    const AugHdr* h = (const AugHdr*)plan;
    const int* bx = (const int*)(plan + h->off_bx);
    const int* kx = (const int*)(plan + h->off_kx);
    fused_draw(d, h, (const int*)(plan + h->off_by), a);
    const int n = blockIdx.y, S = h->image, SV = S >> 2, W3 = h->W * 3, ksx = h->ksx;
    const int y0 = d.ylo + (int)blockIdx.x * rpb;
    if (y0 >= d.yhi || frame_masked(d, a.n_time, n)) return;      // uniform over the block
    const int nrows = d.yhi - y0 < rpb ? d.yhi - y0 : rpb;
    const long row0 = (long)n * h->H + y0;
    const long a0 = row0 * W3, a_al = a0 & ~3L;
    const int head = (int)(a0 - a_al), ndw = (head + nrows * W3 + 3) >> 2;
    for (int i = threadIdx.x; i < ndw; i += VA_THREADS) {
        const long off = a_al + 4L * i;
        unsigned v;
        if (off + 4 <= in_bytes) v = *(const unsigned*)(in + off);
        else { v = 0; for (int e = 0; e < 4 && off + e < in_bytes; ++e) v |= (unsigned)in[off + e] << (8 * e); }
        ((unsigned*)rows_s)[i] = v;
    }
    __syncthreads();
    const int r = threadIdx.x / SV, xo4 = (threadIdx.x - r * SV) * 4;
    if (r >= nrows) return;
    const unsigned char* src = rows_s + head + r * W3;
    unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        const int xo = xo4 + px, c = d.left + (d.flip ? S - 1 - xo : xo);
        const int x0 = bx[2 * c], cnt = bx[2 * c + 1];
        const int* k = kx + (long)c * ksx;
        const unsigned char* p = src + x0 * 3;
        int s0 = 1 << (PBITS - 1), s1 = s0, s2 = s0;
        for (int j = 0; j < cnt; ++j) {
            const int cf = k[j];
            s0 += p[3 * j] * cf; s1 += p[3 * j + 1] * cf; s2 += p[3 * j + 2] * cf;
        }
        const int b0 = 3 * px;
        o[b0 >> 2] |= clip8_lone(s0) << (8 * (b0 & 3));
        o[(b0 + 1) >> 2] |= clip8_lone(s1) << (8 * ((b0 + 1) & 3));
        o[(b0 + 2) >> 2] |= clip8_lone(s2) << (8 * ((b0 + 2) & 3));
    }
    *(uint3*)(tmp + ((row0 + r) * S + xo4) * 3) = make_uint3(o[0], o[1], o[2]);
}

// vertical pass + rescale/normalize: block (x, n) takes 256 of frame n's image * image / VEC output groups.  A masked frame is written as
// `fill` and its tmp rows (which nobody produced) are not read.  Block (0, 0) also leaves info and spans.
template <typename T, int VEC>
__global__ __launch_bounds__(VA_THREADS) void aug_resize_v_norm_kernel(const char* __restrict__ plan, const unsigned char* __restrict__ tmp,
                                                                       T* __restrict__ out, float fill, avllm_video_aug_info* __restrict__ info,
                                                                       int* __restrict__ spans, AugArgs a) {
    __shared__ ClipDraw d;
    const AugHdr* h = (const AugHdr*)plan;
    const int* by = (const int*)(plan + h->off_by);
    const int* ky = (const int*)(plan + h->off_ky);
    const float* lut = (const float*)(plan + h->off_lut);
    fused_draw(d, h, by, a);
    const int n = blockIdx.y, S = h->image, SV = S / VEC;
    if (blockIdx.x == 0 && n == 0) {
        int cnt = 0;
        for (int f0 = 0; f0 < a.N; f0 += VA_THREADS) {
            const int f = f0 + (int)threadIdx.x;
            cnt += __syncthreads_count(f < a.N && frame_masked(d, a.n_time, f));
        }
        if ((int)threadIdx.x < a.n_time) { spans[2 * threadIdx.x] = d.span[threadIdx.x][0]; spans[2 * threadIdx.x + 1] = d.span[threadIdx.x][1]; }
        if (threadIdx.x == 0) {
            avllm_video_aug_info r;
            r.left = d.left; r.top = d.top; r.flip = d.flip; r.masked = cnt;
            *info = r;
        }
    }
    const int i = blockIdx.x * VA_THREADS + threadIdx.x;
    if (i >= S * SV) return;
    const int yo = i / SV, xo = (i - yo * SV) * VEC;
    const long plane = (long)S * S, o = (long)n * 3 * plane + (long)yo * S + xo;
    if (frame_masked(d, a.n_time, n)) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if constexpr (VEC == 4) { const float v[4] = {fill, fill, fill, fill}; store_f<4>(out + o + ch * plane, v); }
            else out[o + ch * plane] = (T)fill;
        }
        return;
    }
    const int yr = d.top + yo, y0 = by[2 * yr], cnt = by[2 * yr + 1];
    const int* k = ky + (long)yr * h->ksy;
    const unsigned char* p = tmp + (((long)n * h->H + y0) * S + xo) * 3;
    int acc[3 * VEC];
#pragma unroll
    for (int e = 0; e < 3 * VEC; ++e) acc[e] = 1 << (PBITS - 1);
    for (int j = 0; j < cnt; ++j) {
        const int c = k[j];
        const unsigned char* q = p + (long)j * S * 3;
        if (VEC == 4) {
            const uint3 w = *(const uint3*)q;                  // 12 bytes, 4-byte aligned (S % 4 == 0)
            const unsigned dw[3] = {w.x, w.y, w.z};
#pragma unroll
            for (int e = 0; e < 12; ++e) acc[e] += (int)((dw[e >> 2] >> (8 * (e & 3))) & 0xffu) * c;
        } else {
#pragma unroll
            for (int e = 0; e < 3; ++e) acc[e] += q[e] * c;
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float v[VEC];
#pragma unroll
        for (int px = 0; px < VEC; ++px) v[px] = lut[ch * 256 + clip8(acc[3 * px + ch])];
        if constexpr (VEC == 4) store_f<4>(out + o + ch * plane, v);
        else out[o + ch * plane] = (T)v[0];
    }
}

// ---------------------------------------------------------------- in place on [B, F, 3, S, S]
// Block (x, b) draws clip first_clip + b with N = nframes[b] and takes work items x 256 + t, ... by grid stride.  An item is one pair of VEC-wide
// groups (g, SV - 1 - g) of one row of one channel plane of one frame below N: both are set to `fill` in a masked frame, exchanged and reversed
// in a flipped one.  The centre element of an odd row maps onto itself and is left alone.  Nothing else is read or written.
template <typename T, int VEC>
__global__ __launch_bounds__(VA_THREADS) void frames_augment_kernel(T* __restrict__ pixels, int F, int S, const int* __restrict__ nframes,
                                                                    int first_clip, float fill, avllm_video_aug_info* __restrict__ info,
                                                                    int* __restrict__ spans, AugArgs a) {
    __shared__ ClipDraw d;
    const int b = blockIdx.y;
    int N = nframes ? nframes[b] : F;
    N = N < 0 ? 0 : (N > F ? F : N);
    clip_draw(d, a, N, (unsigned long long)first_clip + (unsigned long long)b, 1, 1);
    if (blockIdx.x == 0) {
        int cnt = 0;
        for (int f0 = 0; f0 < N; f0 += VA_THREADS) {
            const int f = f0 + (int)threadIdx.x;
            cnt += __syncthreads_count(f < N && frame_masked(d, a.n_time, f));
        }
        if ((int)threadIdx.x < a.n_time) {
            spans[((long)b * a.n_time + threadIdx.x) * 2] = d.span[threadIdx.x][0];
            spans[((long)b * a.n_time + threadIdx.x) * 2 + 1] = d.span[threadIdx.x][1];
        }
        if (threadIdx.x == 0) {
            avllm_video_aug_info r;
            r.left = -1; r.top = -1; r.flip = d.flip; r.masked = cnt;
            info[b] = r;
        }
    }
    const int SV = S / VEC, half = (SV + 1) / 2;
    const long per_frame = 3L * S * half, total = (long)N * per_frame;
    T* clip = pixels + (long)b * F * 3 * S * S;
    for (long i = (long)blockIdx.x * VA_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * VA_THREADS) {
        const int n = (int)(i / per_frame);
        const long rem = i - (long)n * per_frame;
        const long row = rem / half;                            // ch * S + y
        const int g = (int)(rem - row * half), g2 = SV - 1 - g;
        T* r = clip + ((long)n * 3 * S + row) * S;
        if (frame_masked(d, a.n_time, n)) {
            if constexpr (VEC == 4) {
                const float v[4] = {fill, fill, fill, fill};
                store_f<4>(r + 4 * g, v);
                if (g2 != g) store_f<4>(r + 4 * g2, v);
            } else {
                r[g] = (T)fill;
                if (g2 != g) r[g2] = (T)fill;
            }
        } else if (d.flip) {
            if constexpr (VEC == 4) {
                typedef T V4 __attribute__((ext_vector_type(4)));      // 16 bytes (fp32) or 8 (bf16), moved as bits
                const V4 lo = *(const V4*)(r + 4 * g), hi = *(const V4*)(r + 4 * g2);
                *(V4*)(r + 4 * g) = hi.wzyx;
                if (g2 != g) *(V4*)(r + 4 * g2) = lo.wzyx;
            } else if (g2 != g) {
                const T lo = r[g], hi = r[g2];
                r[g] = hi; r[g2] = lo;
            }
        }
    }
}

size_t aug_plan_layout(int H, int W, int resize, int image, AugHdr& h) {
    int nh, nw;
    resized_shape(H, W, resize, nh, nw);
    h.H = H; h.W = W; h.resize = resize; h.image = image; h.newH = nh; h.newW = nw;
    h.ksx = coeff_ksize(W, nw); h.ksy = coeff_ksize(H, nh);
    size_t off = (sizeof(AugHdr) + 15) & ~(size_t)15;
    h.off_bx = (int)off; off += (size_t)nw * 2 * 4;
    h.off_kx = (int)off; off += (size_t)nw * h.ksx * 4;
    h.off_by = (int)off; off += (size_t)nh * 2 * 4;
    h.off_ky = (int)off; off += (size_t)nh * h.ksy * 4;
    h.off_lut = (int)off; off += 3 * 256 * 4;
    return (off + 255) & ~(size_t)255;
}

// plans this process initialised: the compute call checks its (H, W, resize, image) against the plan it is handed
std::mutex g_aug_plan_mu;
std::map<const void*, std::array<int, 4>> g_aug_plans;

inline uint32_t prob24(float p) { return (uint32_t)((double)p * 16777216.0 + 0.5); }      // round(p 2^24) of the float argument, in double: exact

// the checks the two entries share; 0 when the mask arguments are usable
int check_masks(const char* who, float p_flip, int32_t n_time, int32_t max_time_width, float max_time_ratio) {
    AV_CHECK_ARG(n_time >= 0 && n_time <= VA_MAX_MASKS, "%s: n_time=%d masks: at least 0, at most %d", who, n_time, VA_MAX_MASKS);
    AV_CHECK_ARG(max_time_width >= 0, "%s: max_time_width=%d must be at least 0", who, max_time_width);
    AV_CHECK_ARG(p_flip >= 0.f && p_flip <= 1.f, "%s: p_flip=%g must lie in [0, 1]", who, (double)p_flip);
    AV_CHECK_ARG(max_time_ratio >= 0.f && max_time_ratio <= 1.f, "%s: max_time_ratio=%g must lie in [0, 1]", who, (double)max_time_ratio);
    return AV_OK;
}

}  // namespace

// =============================================================================================== C ABI
extern "C" size_t avllm_clip_preproc_aug_plan_bytes(int32_t H, int32_t W, int32_t resize, int32_t image) {
    if (H <= 0 || W <= 0 || image <= 0 || resize < image) return 0;
    AugHdr h;
    return aug_plan_layout(H, W, resize, image, h);
}

extern "C" int avllm_clip_preproc_aug_plan_init(void* plan_dev, int32_t H, int32_t W, int32_t resize, int32_t image, const float* mean3,
                                                const float* std3) {
    AV_CHECK_ARG(plan_dev && mean3 && std3 && H > 0 && W > 0 && image > 0, "clip_preproc_aug_plan_init: null/empty");
    AV_CHECK_ARG(resize >= image, "clip_preproc_aug_plan_init: resize=%d < image=%d: the crop window must fit the resized frame", resize, image);
    AugHdr h;
    const size_t bytes = aug_plan_layout(H, W, resize, image, h);
    std::vector<char> buf(bytes, 0);
    std::vector<int> b, k;
    coeffs(W, h.newW, 0, h.newW, b, k, h.ksx);
    memcpy(buf.data() + h.off_bx, b.data(), b.size() * 4); memcpy(buf.data() + h.off_kx, k.data(), k.size() * 4);
    coeffs(H, h.newH, 0, h.newH, b, k, h.ksy);
    memcpy(buf.data() + h.off_by, b.data(), b.size() * 4); memcpy(buf.data() + h.off_ky, k.data(), k.size() * 4);
    normalize_lut(mean3, std3, (float*)(buf.data() + h.off_lut));
    memcpy(buf.data(), &h, sizeof(h));
    AV_HIP(hipMemcpy(plan_dev, buf.data(), bytes, hipMemcpyHostToDevice));
    { std::lock_guard<std::mutex> lk(g_aug_plan_mu); g_aug_plans[plan_dev] = {H, W, resize, image}; }
    return AV_OK;
}

extern "C" size_t avllm_clip_preproc_aug_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t resize, int32_t image) {
    (void)W; (void)resize;
    if (N <= 0 || H <= 0 || image <= 0) return 0;
    return (size_t)N * H * image * 3 + 256;
}

extern "C" int avllm_clip_preproc_aug(const void* plan, const uint8_t* frames, int32_t N, int32_t H, int32_t W, int32_t resize, int32_t image,
                                      int32_t clip, int32_t random_crop, float p_flip, int32_t n_time, int32_t max_time_width,
                                      float max_time_ratio, float fill, uint32_t seed, const uint32_t* seed_dev, void* out, int32_t dtype,
                                      avllm_video_aug_info* info, int32_t* spans, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AV_CHECK_ARG(plan && frames && out && info && N > 0 && N <= 65535 && H > 0 && W > 0 && image > 0,
                 "clip_preproc_aug: bad args (plan %s, frames %s, out %s, info %s, N=%d H=%d W=%d image=%d)", plan ? "set" : "NULL",
                 frames ? "set" : "NULL", out ? "set" : "NULL", info ? "set" : "NULL", N, H, W, image);
    AV_CHECK_ARG(resize >= image, "clip_preproc_aug: resize=%d < image=%d: the crop window must fit the resized frame", resize, image);
    AV_TRY(check_masks("clip_preproc_aug", p_flip, n_time, max_time_width, max_time_ratio));
    AV_CHECK_ARG(n_time == 0 || spans, "clip_preproc_aug: spans is NULL with n_time=%d", n_time);
    AV_CHECK_ARG(clip >= 0, "clip_preproc_aug: clip=%d must be at least 0", clip);
    AV_CHECK_ARG(dtype == AV_F32 || dtype == AV_BF16, "clip_preproc_aug: dtype %d", dtype);
    AV_CHECK_ARG((long)N * H * W * 3 < (1L << 40) && (long)H * image < (1L << 31), "clip_preproc_aug: batch too large");
    {
        std::lock_guard<std::mutex> lk(g_aug_plan_mu);
        auto it = g_aug_plans.find(plan);
        AV_CHECK_ARG(it != g_aug_plans.end(), "clip_preproc_aug: plan was not initialised with avllm_clip_preproc_aug_plan_init");
        AV_CHECK_ARG(it->second[0] == H && it->second[1] == W && it->second[2] == resize && it->second[3] == image,
                     "clip_preproc_aug: plan is for %dx%d->%d->%d, call is %dx%d->%d->%d", it->second[0], it->second[1], it->second[2],
                     it->second[3], H, W, resize, image);
    }
    const size_t need = avllm_clip_preproc_aug_workspace_bytes(N, H, W, resize, image);
    AV_CHECK_ARG(ws && ws_bytes >= need, "clip_preproc_aug: workspace too small (%zu bytes given, %zu needed)", ws ? ws_bytes : (size_t)0, need);
    AugArgs a;
    a.N = N; a.clip = clip; a.random_crop = random_crop != 0; a.n_time = n_time; a.max_tw = max_time_width; a.ratio = max_time_ratio;
    a.thr = prob24(p_flip); a.seed = seed; a.seed_dev = seed_dev;
    unsigned char* tmp = (unsigned char*)ws;
    const char* pl = (const char*)plan;
    const int rpb = image % 4 == 0 && image <= 1024 ? VA_THREADS / (image / 4) : 0;
    if (rpb > 0 && (size_t)rpb * W * 3 + 8 <= 60 * 1024) {
        const size_t lds = ((size_t)rpb * W * 3 + 8 + 15) & ~(size_t)15;
        hipLaunchKernelGGL(aug_resize_h4_kernel, dim3(av_cdiv(H, rpb), N), dim3(VA_THREADS), lds, st, pl, frames, tmp, (long)N * H * W * 3, rpb, a);
    } else {
        hipLaunchKernelGGL(aug_resize_h_kernel, dim3(av_cdiv((long)H * image, VA_THREADS), N), dim3(VA_THREADS), 0, st, pl, frames, tmp, a);
    }
    AV_LAUNCH_CHECK();
    if (image % 4 == 0) {
        const dim3 grid(av_cdiv(image * (image / 4), VA_THREADS), N);
        if (dtype == AV_F32) hipLaunchKernelGGL((aug_resize_v_norm_kernel<float, 4>), grid, dim3(VA_THREADS), 0, st, pl, tmp, (float*)out, fill, info, spans, a);
        else hipLaunchKernelGGL((aug_resize_v_norm_kernel<bf16, 4>), grid, dim3(VA_THREADS), 0, st, pl, tmp, (bf16*)out, fill, info, spans, a);
    } else {
        const dim3 grid(av_cdiv((long)image * image, VA_THREADS), N);
        if (dtype == AV_F32) hipLaunchKernelGGL((aug_resize_v_norm_kernel<float, 1>), grid, dim3(VA_THREADS), 0, st, pl, tmp, (float*)out, fill, info, spans, a);
        else hipLaunchKernelGGL((aug_resize_v_norm_kernel<bf16, 1>), grid, dim3(VA_THREADS), 0, st, pl, tmp, (bf16*)out, fill, info, spans, a);
    }
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int avllm_video_frames_augment(void* pixels, int32_t dtype, int32_t B, int32_t F, int32_t image, const int32_t* nframes,
                                          int32_t first_clip, float p_flip, int32_t n_time, int32_t max_time_width, float max_time_ratio,
                                          float fill, uint32_t seed, const uint32_t* seed_dev, avllm_video_aug_info* info, int32_t* spans,
                                          void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AV_TRY(check_masks("video_frames_augment", p_flip, n_time, max_time_width, max_time_ratio));
    AV_CHECK_ARG(first_clip >= 0, "video_frames_augment: first_clip=%d must be at least 0", first_clip);
    AugArgs a;
    a.N = 0; a.clip = first_clip; a.random_crop = 0; a.n_time = n_time; a.max_tw = max_time_width; a.ratio = max_time_ratio;
    a.thr = prob24(p_flip); a.seed = seed; a.seed_dev = seed_dev;
    if (a.thr == 0 && n_time == 0) return AV_OK;
    AV_CHECK_ARG(pixels && info && (n_time == 0 || spans) && B > 0 && B <= 65535 && F > 0 && image > 0,
                 "video_frames_augment: bad args (pixels %s, info %s, spans %s, B=%d F=%d image=%d)", pixels ? "set" : "NULL",
                 info ? "set" : "NULL", spans ? "set" : "NULL", B, F, image);
    AV_CHECK_ARG(dtype == AV_F32 || dtype == AV_BF16, "video_frames_augment: dtype %d", dtype);
    AV_CHECK_ARG((long)F * 3 * image * image < (1L << 40), "video_frames_augment: clip too large");
    const bool vec = image % 4 == 0 && (uintptr_t)pixels % 16 == 0;
    const long items = (long)F * 3 * image * ((image / (vec ? 4 : 1) + 1) / 2);
    const long want = av_cdiv(items, VA_THREADS);
    const int cap = VA_MAX_BLOCKS / B > 1 ? VA_MAX_BLOCKS / B : 1;
    const dim3 grid((unsigned)(want < cap ? want : cap), B), block(VA_THREADS);
    if (dtype == AV_F32) {
        if (vec) hipLaunchKernelGGL((frames_augment_kernel<float, 4>), grid, block, 0, st, (float*)pixels, F, image, nframes, first_clip, fill, info, spans, a);
        else hipLaunchKernelGGL((frames_augment_kernel<float, 1>), grid, block, 0, st, (float*)pixels, F, image, nframes, first_clip, fill, info, spans, a);
    } else {
        if (vec) hipLaunchKernelGGL((frames_augment_kernel<bf16, 4>), grid, block, 0, st, (bf16*)pixels, F, image, nframes, first_clip, fill, info, spans, a);
        else hipLaunchKernelGGL((frames_augment_kernel<bf16, 1>), grid, block, 0, st, (bf16*)pixels, F, image, nframes, first_clip, fill, info, spans, a);
    }
    AV_LAUNCH_CHECK();
    return AV_OK;
}
