// Acoustic augmentation on the device (include/avllm.h, "acoustic augmentation"): avllm_wave_add_noise mixes one segment of a noise bank into
// each clip at a requested SNR, avllm_spec_augment masks time and frequency spans of a feature tensor.  Both rules are stated in full in the
// header and restated on the host by tests/refs64_augment.py.  Nothing on the default path comes here.
#include "common.h"
#include "avllm_internal.h"
#include <math.h>

constexpr int AUG_THREADS = 256;
constexpr int AUG_CHUNK = 4096;                 // samples per energy partial (avllm_wave_add_noise_chunk): 4 float4 per thread
constexpr int AUG_MAX_BLOCKS = 2048;            // memory-bound: a few blocks per CU, the rest by grid stride
constexpr uint32_t NOISE_SALT = 0x6E6F6973u;    // "nois"
constexpr uint32_t SPEC_SALT = 0x73706563u;     // "spec"
constexpr int SPEC_MAX_MASKS = 32;

// a * b + c with the product rounded before the sum.  HIP's __fmul_rn / __fadd_rn are plain operators the compiler may still contract into an
// fma; the pragma is what keeps the two roundings the header promises and the host restates.
template <typename T> __device__ __forceinline__ T unfused_madd(T a, T b, T c) {
#pragma clang fp contract(off)
    const T p = a * b;
    return p + c;
}

// ---------------------------------------------------------------- the draw of one clip
struct NoiseDraw { int hit, row, offset, nl, len; float snr; };

__device__ __forceinline__ NoiseDraw noise_draw(int b, const int* len, int n, const int* noise_len, int Nn, long ld_noise, const float* snr_db,
                                                float lo, float hi, uint32_t thr, uint32_t seed, const uint32_t* seed_dev) {
    NoiseDraw d;
    const uint32_t s = av_seed(seed_dev, seed) + NOISE_SALT;
    const unsigned long long k = 4ull * (unsigned long long)b;
    const uint32_t h0 = av_pair_hash(s, k), h1 = av_pair_hash(s, k + 1), h2 = av_pair_hash(s, k + 2), h3 = av_pair_hash(s, k + 3);
    int l = len ? len[b] : n;
    d.len = l < 0 ? 0 : (l > n ? n : l);
    d.hit = (h0 >> 8) < thr && d.len > 0;
    d.row = (int)(((unsigned long long)h1 * (unsigned long long)Nn) >> 32);
    long nl = noise_len[d.row];
    nl = nl < 1 ? 1 : (nl > ld_noise ? ld_noise : nl);        // a length outside [1, ld_noise] is read as the nearest bound: no read leaves the row
    d.nl = (int)nl;
    d.offset = (int)(((unsigned long long)h2 * (unsigned long long)d.nl) >> 32);
    // lo + (hi - lo) * u with u = (h3 >> 8) * 2^-24 exact; one product and one sum, each rounded once (no fused form: the host restates it)
    d.snr = snr_db ? snr_db[b] : (float)unfused_madd((double)hi - (double)lo, (double)(h3 >> 8) * (1.0 / 16777216.0), (double)lo);
    return d;
}

// ---------------------------------------------------------------- energies
// Block (x, b) takes chunks x, x + gridDim.x, ... of clip b below len_b and leaves {Es, En} of each in part[b][chunk].  Thread t of a chunk owns
// elements 4 (t + 256 k) + 0..3, k = 0..3, in both the 16-byte and the scalar form, adds them in that order, and the block folds lanes then
// waves in a fixed tree: the bits of a partial depend on nothing but the data.  Elements at or past len_b are not loaded into a sum.
template <bool VEC>
__global__ void __launch_bounds__(AUG_THREADS) noise_energy_kernel(const float* wave, long ld, const int* len, int n, const float* __restrict__ noise,
                                                                   long ld_noise, const int* __restrict__ noise_len, int Nn, uint32_t thr,
                                                                   uint32_t seed, const uint32_t* seed_dev, double* __restrict__ part, int nchunk) {
    const int b = blockIdx.y;
    const NoiseDraw d = noise_draw(b, len, n, noise_len, Nn, ld_noise, nullptr, 0.f, 0.f, thr, seed, seed_dev);
    if (!d.hit) return;
    const float* w = wave + (long)b * ld;
    const float* z = noise + (long)d.row * ld_noise;
    const int nc = (d.len + AUG_CHUNK - 1) / AUG_CHUNK;
    __shared__ double red[2][AUG_THREADS / 64];
    for (int c = blockIdx.x; c < nc; c += gridDim.x) {
        double es = 0.0, en = 0.0;
#pragma unroll
        for (int k = 0; k < AUG_CHUNK / (4 * AUG_THREADS); ++k) {
            const int i = c * AUG_CHUNK + 4 * ((int)threadIdx.x + AUG_THREADS * k);
            if (i >= d.len) continue;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            const int m = d.len - i < 4 ? d.len - i : 4;
            if (VEC && m == 4) { const float4 q = *reinterpret_cast<const float4*>(w + i); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
            else for (int e = 0; e < m; ++e) v[e] = w[i + e];
            uint32_t pos = ((uint32_t)d.offset + (uint32_t)i) % (uint32_t)d.nl;
            for (int e = 0; e < m; ++e) {
                const double zv = (double)z[pos], wv = (double)v[e];
                es += wv * wv; en += zv * zv;
                if (++pos >= (uint32_t)d.nl) pos = 0;
            }
        }
        for (int o = 32; o > 0; o >>= 1) { es += __shfl_down(es, o); en += __shfl_down(en, o); }
        const int wv_ = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { red[0][wv_] = es; red[1][wv_] = en; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double a = red[0][0], e2 = red[1][0];
            for (int q = 1; q < AUG_THREADS / 64; ++q) { a += red[0][q]; e2 += red[1][q]; }
            part[((long)b * nchunk + c) * 2] = a;
            part[((long)b * nchunk + c) * 2 + 1] = e2;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- mix
// Block (x, b) folds clip b's partials in index order (every thread the same uniform loop), forms the gain, then takes chunks x, x + gridDim.x,
// ... of the whole row: w + gain z below len_b (a product and a sum, each rounded to float), a copy of the bits from there on.  A clip that is
// not mixed is copied, or left alone when out is wave.  Each element is read and written by one thread, so out may be wave.
template <bool VEC>
__global__ void __launch_bounds__(AUG_THREADS) noise_mix_kernel(const float* wave, long ld, const int* len, int n, const float* __restrict__ noise,
                                                                long ld_noise, const int* __restrict__ noise_len, int Nn,
                                                                const float* __restrict__ snr_db, float lo, float hi, uint32_t thr, uint32_t seed,
                                                                const uint32_t* seed_dev, const double* __restrict__ part, int nchunk, float* out,
                                                                long ld_out, avllm_noise_info* __restrict__ info) {
    const int b = blockIdx.y;
    const NoiseDraw d = noise_draw(b, len, n, noise_len, Nn, ld_noise, snr_db, lo, hi, thr, seed, seed_dev);
    float gain = 0.f;
    if (d.hit) {
        double es = 0.0, en = 0.0;
        const int nc = (d.len + AUG_CHUNK - 1) / AUG_CHUNK;
        for (int c = 0; c < nc; ++c) { es += part[((long)b * nchunk + c) * 2]; en += part[((long)b * nchunk + c) * 2 + 1]; }
        if (es > 0.0 && en > 0.0 && es < INFINITY && en < INFINITY) {
            const float g = (float)sqrt(es / (en * pow(10.0, (double)d.snr / 10.0)));
            if (g > 0.f && g < INFINITY) gain = g;
        }
    }
    const bool mixed = gain != 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        avllm_noise_info r;
        r.applied = mixed ? 1 : 0; r.row = d.row; r.offset = d.offset; r.snr_db = d.snr; r.gain = gain;
        info[b] = r;
    }
    const float* w = wave + (long)b * ld;
    float* o = out + (long)b * ld_out;
    if (!mixed && o == w) return;
    const float* z = noise + (long)d.row * ld_noise;
    const int lim = mixed ? d.len : 0;
    const int nc = (n + AUG_CHUNK - 1) / AUG_CHUNK;
    for (int c = blockIdx.x; c < nc; c += gridDim.x) {
#pragma unroll
        for (int k = 0; k < AUG_CHUNK / (4 * AUG_THREADS); ++k) {
            const int i = c * AUG_CHUNK + 4 * ((int)threadIdx.x + AUG_THREADS * k);
            if (i >= n) continue;
            float v[4];
            const int m = n - i < 4 ? n - i : 4;
            if (VEC && m == 4) { const float4 q = *reinterpret_cast<const float4*>(w + i); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
            else for (int e = 0; e < m; ++e) v[e] = w[i + e];
            if (i < lim) {
                uint32_t pos = ((uint32_t)d.offset + (uint32_t)i) % (uint32_t)d.nl;
                for (int e = 0; e < m && i + e < lim; ++e) {
                    v[e] = unfused_madd(gain, z[pos], v[e]);
                    if (++pos >= (uint32_t)d.nl) pos = 0;
                }
            }
            if (VEC && m == 4) *reinterpret_cast<float4*>(o + i) = make_float4(v[0], v[1], v[2], v[3]);
            else for (int e = 0; e < m; ++e) o[i + e] = v[e];
        }
    }
}

static inline uint32_t prob24(float p) { return (uint32_t)((double)p * 16777216.0 + 0.5); }      // round(p 2^24) of the float argument, in double: exact
static inline int capped_x(int want, int B) {
    const int cap = AUG_MAX_BLOCKS / B > 1 ? AUG_MAX_BLOCKS / B : 1;
    return want < 1 ? 1 : (want < cap ? want : cap);
}

extern "C" int32_t avllm_wave_add_noise_chunk(void) { return AUG_CHUNK; }

extern "C" size_t avllm_wave_add_noise_workspace_bytes(int32_t B, int32_t n) {
    if (B <= 0 || n <= 0) return 0;
    return (size_t)B * (size_t)((n + AUG_CHUNK - 1) / AUG_CHUNK) * 2 * sizeof(double);
}

extern "C" int avllm_wave_add_noise(const float* wave, int64_t ld, const int32_t* len, int32_t B, int32_t n, const float* noise, int64_t ld_noise,
                                    const int32_t* noise_len, int32_t Nn, const float* snr_db, float snr_lo, float snr_hi, float p_apply,
                                    uint32_t seed, const uint32_t* seed_dev, float* out, int64_t ld_out, avllm_noise_info* info, void* ws,
                                    size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AV_CHECK_ARG(wave && out && info && B > 0 && B <= 65535 && n > 0 && n <= (1 << 30) && ld >= n && ld_out >= n,
                 "wave_add_noise: bad args (wave %s, out %s, info %s, B=%d n=%d ld=%ld ld_out=%ld)", wave ? "set" : "NULL", out ? "set" : "NULL",
                 info ? "set" : "NULL", B, n, (long)ld, (long)ld_out);
    AV_CHECK_ARG(out != wave || ld_out == ld, "wave_add_noise: out aliases wave with another row stride (ld=%ld ld_out=%ld)", (long)ld, (long)ld_out);
    AV_CHECK_ARG(Nn > 0, "wave_add_noise: Nn=%d: the noise bank needs at least one row", Nn);
    AV_CHECK_ARG(noise && noise_len && ld_noise >= 1, "wave_add_noise: noise bank (noise %s, noise_len %s, ld_noise=%ld)", noise ? "set" : "NULL",
                 noise_len ? "set" : "NULL", (long)ld_noise);
    AV_CHECK_ARG(p_apply >= 0.f && p_apply <= 1.f, "wave_add_noise: p_apply=%g must lie in [0, 1]", (double)p_apply);
    AV_CHECK_ARG(snr_db || (snr_lo <= snr_hi && snr_lo > -INFINITY && snr_hi < INFINITY),
                 "wave_add_noise: snr_lo=%g > snr_hi=%g (or not finite): without snr_db the range must be ordered", (double)snr_lo, (double)snr_hi);
    const size_t need = avllm_wave_add_noise_workspace_bytes(B, n);
    AV_CHECK_ARG(ws && ws_bytes >= need && (uintptr_t)ws % 8 == 0, "wave_add_noise: workspace too small or misaligned (%zu bytes given, %zu needed, 8-byte aligned)",
                 ws ? ws_bytes : (size_t)0, need);
    const int nchunk = (n + AUG_CHUNK - 1) / AUG_CHUNK;
    const uint32_t thr = prob24(p_apply);
    const dim3 grid(capped_x(nchunk, B), B), block(AUG_THREADS);
    const bool vec = (uintptr_t)wave % 16 == 0 && (uintptr_t)out % 16 == 0 && ld % 4 == 0 && ld_out % 4 == 0;
    double* part = (double*)ws;
    if (thr) {      // p_apply = 0: no clip is mixed, no energy is needed
        if (vec) hipLaunchKernelGGL((noise_energy_kernel<true>), grid, block, 0, st, wave, (long)ld, len, n, noise, (long)ld_noise, noise_len, Nn, thr, seed, seed_dev, part, nchunk);
        else hipLaunchKernelGGL((noise_energy_kernel<false>), grid, block, 0, st, wave, (long)ld, len, n, noise, (long)ld_noise, noise_len, Nn, thr, seed, seed_dev, part, nchunk);
        AV_LAUNCH_CHECK();
    }
    if (vec) hipLaunchKernelGGL((noise_mix_kernel<true>), grid, block, 0, st, wave, (long)ld, len, n, noise, (long)ld_noise, noise_len, Nn, snr_db, snr_lo, snr_hi, thr, seed, seed_dev, part, nchunk, out, (long)ld_out, info);
    else hipLaunchKernelGGL((noise_mix_kernel<false>), grid, block, 0, st, wave, (long)ld, len, n, noise, (long)ld_noise, noise_len, Nn, snr_db, snr_lo, snr_hi, thr, seed, seed_dev, part, nchunk, out, (long)ld_out, info);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

// ---------------------------------------------------------------- SpecAugment
// Block (x, b) recomputes clip b's spans into LDS (thread j: mask j), then takes rows x, x + gridDim.x, ... of the clip: a row inside a frequency
// span is filled over all T frames, any other row over the time spans only.  Only masked cells are written (and none is read), so every other
// cell keeps its bits; spans that overlap write the same value twice.
__global__ void __launch_bounds__(AUG_THREADS) spec_augment_kernel(float* __restrict__ feat, int M, int T, const int* __restrict__ valid, int n_time,
                                                                   int max_tw, float ratio, int n_freq, int max_fw, float fill, uint32_t seed,
                                                                   const uint32_t* seed_dev, int* __restrict__ spans) {
    __shared__ int sp[SPEC_MAX_MASKS][2];
    const int b = blockIdx.y, nm = n_time + n_freq;
    if ((int)threadIdx.x < nm) {
        const int j = threadIdx.x;
        const uint32_t s = av_seed(seed_dev, seed) + SPEC_SALT;
        const unsigned long long k = 64ull * (unsigned long long)b + 2ull * (unsigned long long)j;
        const uint32_t h = av_pair_hash(s, k), h2 = av_pair_hash(s, k + 1);
        int extent, wmax;
        if (j < n_time) {
            const int v = valid ? valid[b] : T;
            extent = v < 0 ? 0 : (v > T ? T : v);
            const double cap = floor((double)ratio * (double)extent);
            wmax = (double)max_tw < cap ? max_tw : (int)cap;
        } else {
            extent = M;
            wmax = max_fw < M ? max_fw : M;
        }
        const int w = (int)(((unsigned long long)h * (unsigned long long)(wmax + 1)) >> 32);
        const int start = (int)(((unsigned long long)h2 * (unsigned long long)(extent - w + 1)) >> 32);
        sp[j][0] = start; sp[j][1] = w;
        if (blockIdx.x == 0) { spans[((long)b * nm + j) * 2] = start; spans[((long)b * nm + j) * 2 + 1] = w; }
    }
    __syncthreads();
    for (int m = blockIdx.x; m < M; m += gridDim.x) {
        float* row = feat + ((long)b * M + m) * T;
        bool whole = false;
        for (int j = n_time; j < nm; ++j) whole |= m >= sp[j][0] && m < sp[j][0] + sp[j][1];
        if (whole) {
            for (int t = threadIdx.x; t < T; t += AUG_THREADS) row[t] = fill;
        } else {
            for (int j = 0; j < n_time; ++j) {
                const int s0 = sp[j][0], w = sp[j][1];
                for (int t = threadIdx.x; t < w; t += AUG_THREADS) row[s0 + t] = fill;
            }
        }
    }
}

extern "C" int avllm_spec_augment(float* feat, int32_t B, int32_t M, int32_t T, const int32_t* valid, int32_t n_time, int32_t max_time_width,
                                  float max_time_ratio, int32_t n_freq, int32_t max_freq_width, float fill, uint32_t seed, const uint32_t* seed_dev,
                                  int32_t* spans, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AV_CHECK_ARG(n_time >= 0 && n_freq >= 0 && n_time + n_freq <= SPEC_MAX_MASKS, "spec_augment: n_time=%d + n_freq=%d masks: each at least 0, at most %d together",
                 n_time, n_freq, SPEC_MAX_MASKS);
    AV_CHECK_ARG(max_time_width >= 0 && max_freq_width >= 0, "spec_augment: max_time_width=%d and max_freq_width=%d must be at least 0", max_time_width, max_freq_width);
    AV_CHECK_ARG(max_time_ratio >= 0.f && max_time_ratio <= 1.f, "spec_augment: max_time_ratio=%g must lie in [0, 1]", (double)max_time_ratio);
    if (n_time + n_freq == 0) return AV_OK;
    AV_CHECK_ARG(feat && spans && B > 0 && B <= 65535 && M > 0 && T > 0, "spec_augment: bad args (feat %s, spans %s, B=%d M=%d T=%d)", feat ? "set" : "NULL",
                 spans ? "set" : "NULL", B, M, T);
    hipLaunchKernelGGL(spec_augment_kernel, dim3(capped_x(M, B), B), dim3(AUG_THREADS), 0, st, feat, M, T, valid, n_time, max_time_width, max_time_ratio,
                       n_freq, max_freq_width, fill, seed, seed_dev, spans);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
