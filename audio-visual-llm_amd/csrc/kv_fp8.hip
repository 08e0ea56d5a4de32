// KV cache in block-scaled e4m3 (OCP MX: one E8M0 exponent, biased by 127, per 32 consecutive elements of a cache row) for the fused token step.
// A cache row of dkv bf16 values becomes dkv codes + dkv/32 exponent bytes, 33/64 of its bytes, by the rule of mx.h (amax == 0 -> byte 0).
// Blocks never straddle a head (hd is 64 or 128).  A cache image is two planes: the codes of every row first ([..., dkv] bytes, rows 64-byte
// multiples so a lane's 16 codes are one aligned 16-byte load), then the exponents ([..., dkv/32] bytes); the kernels take the two plane
// pointers of a layer.  This file writes and moves the image; the token step reads it in attention_decode.hip (the e4m3 row form).
//
//   kv8_append_kernel        prefill: rows [B, S] of the rotated k and of v in the q|k|v buffer -> codes + exponents at [pos0, pos0 + S)
//   kv8_rope_append_kernel   token step, after the raw q|k|v projection: rotates q in place (fp32, one rounding to bf16), rotates k (fp32, no
//                            bf16 rounding in between), quantises k and v and writes the row at pos (+ *pos_dev); rotate = 0 after a head-norm
//                            launch that has rotated already (Qwen3)
// The beam-search gather moves both planes with the byte-row form of kv_gather_rows (beam.hip): rows of dkv and of dkv/32 bytes.
#include "common.h"
#include "avllm_internal.h"
#include "mx.h"

namespace {

struct Kv8Planes { uint8_t *kq, *ke, *vq, *ve; };       // codes [B, Tmax, dkv], exponents [B, Tmax, dkv/32] of K and of V

// one thread = one block of 32 of one appended row of K or V
__global__ __launch_bounds__(256) void kv8_append_kernel(const bf16* __restrict__ k, const bf16* __restrict__ v, long ld, Kv8Planes c, int B, int Tn,
                                                         int pos0, int Tmax, int dkv) {
    const int nb = dkv >> 5;
    const long half = (long)B * Tn * nb, total = 2 * half;
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const bool isv = idx >= half;
        const long i = isv ? idx - half : idx;
        const int blk = (int)(i % nb);
        const long row = i / nb;
        const int b = (int)(row / Tn), t = (int)(row % Tn);
        float x[32];
        mx_load32((isv ? v : k) + row * ld + blk * 32, x);
        const long crow = (long)b * Tmax + pos0 + t;
        mx_block32_store(x, (isv ? c.vq : c.kq) + crow * dkv + blk * 32, (isv ? c.ve : c.ke) + crow * nb + blk);
    }
}

struct Kv8RopeArgs {
    bf16* qkv; long ld;                 // [B, ld]: q [H hd] | k [Hkv hd] | v [Hkv hd], raw (rotate) or with q and k already rotated
    int B, H, Hkv, hd, rotate;
    const float* rope;                  // [hd/2][2] cos, sin of the step's position
    Kv8Planes c; int Tmax, pos; const int* pos_dev;
};
// Work items of a row, in this order: q (rotate only) 8 rotary pairs each; k one pair of partner blocks (elements [32 j, 32 j + 32) of a head and
// the 32 at + hd/2) each; v one block each.
__global__ __launch_bounds__(256) void kv8_rope_append_kernel(Kv8RopeArgs a) {
    const int hd = a.hd, hh = hd >> 1, d = a.H * hd, dkv = a.Hkv * hd, nb = dkv >> 5;
    const int nq = a.rotate ? a.H * (hd >> 4) : 0, nk = a.Hkv * (hd >> 6), nv = nb, per = nq + nk + nv;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.B * per) return;
    const int b = idx / per, it = idx - b * per;
    bf16* row = a.qkv + (long)b * a.ld;
    if (it < nq) {
        const int h = it / (hd >> 4), c0 = (it - h * (hd >> 4)) * 8;
        bf16* lo = row + h * hd + c0;
        float x[8], y[8], ox[8], oy[8];
        load_f<8>(lo, x);
        load_f<8>(lo + hh, y);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float cs = a.rope[2 * (c0 + e)], sn = a.rope[2 * (c0 + e) + 1];
            ox[e] = x[e] * cs - y[e] * sn;
            oy[e] = y[e] * cs + x[e] * sn;
        }
        store_f<8>(lo, ox);
        store_f<8>(lo + hh, oy);
        return;
    }
    // position from device memory: the host could not check it.  A step replayed past the end of the cache writes nothing (dec_proj's rule)
    const int pos = a.pos + (a.pos_dev ? *a.pos_dev : 0);
    if (pos < 0 || pos >= a.Tmax) return;
    const long crow = (long)b * a.Tmax + pos;
    if (it < nq + nk) {
        const int i = it - nq, hk = i / (hd >> 6), j = i - hk * (hd >> 6), c0 = hk * hd + 32 * j;
        float x[32], y[32];
        mx_load32(row + d + c0, x);
        mx_load32(row + d + c0 + hh, y);
        if (a.rotate) {
#pragma unroll
            for (int e = 0; e < 32; ++e) {
                const float cs = a.rope[2 * (32 * j + e)], sn = a.rope[2 * (32 * j + e) + 1];
                const float ox = x[e] * cs - y[e] * sn, oy = y[e] * cs + x[e] * sn;
                x[e] = ox; y[e] = oy;
            }
        }
        mx_block32_store(x, a.c.kq + crow * dkv + c0, a.c.ke + crow * nb + (c0 >> 5));
        mx_block32_store(y, a.c.kq + crow * dkv + c0 + hh, a.c.ke + crow * nb + ((c0 + hh) >> 5));
        return;
    }
    const int blk = it - nq - nk;
    float x[32];
    mx_load32(row + d + dkv + blk * 32, x);
    mx_block32_store(x, a.c.vq + crow * dkv + blk * 32, a.c.ve + crow * nb + blk);
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int av_kv8_append(const void* k, const void* v, long ld, void* kq, void* ke, void* vq, void* ve, int B, int T, int pos0, int Tmax, int dkv, hipStream_t st) {
    AV_CHECK_ARG(k && v && kq && ke && vq && ve && B > 0 && T > 0 && pos0 >= 0 && pos0 + T <= Tmax, "kv8_append: bad args (pos0=%d T=%d Tmax=%d)", pos0, T, Tmax);
    AV_CHECK_ARG(dkv > 0 && dkv % 32 == 0 && ld % 8 == 0 && ld >= dkv && al16(k) && al16(v) && al16(kq) && al16(vq),
                 "kv8_append: dkv=%d must be a multiple of 32, rows (ld=%ld) and code planes 16-byte aligned", dkv, ld);
    const long total = 2L * B * T * (dkv >> 5);
    long blocks = (total + 255) / 256;
    blocks = blocks > 65536 ? 65536 : blocks;
    hipLaunchKernelGGL(kv8_append_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const bf16*)k, (const bf16*)v, ld,
                       Kv8Planes{(uint8_t*)kq, (uint8_t*)ke, (uint8_t*)vq, (uint8_t*)ve}, B, T, pos0, Tmax, dkv);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_kv8_rope_append(void* qkv, long ld, int B, int H, int Hkv, int hd, const float* rope, int rotate, void* kq, void* ke, void* vq, void* ve, int Tmax,
                       int pos, const int* pos_dev, hipStream_t st) {
    AV_CHECK_ARG(qkv && kq && ke && vq && ve && B > 0 && H > 0 && Hkv > 0 && (rope || !rotate), "kv8_rope_append: null/empty");
    AV_CHECK_ARG(hd == 64 || hd == 128, "kv8_rope_append: head_dim %d (64 or 128)", hd);
    AV_CHECK_ARG(ld % 8 == 0 && ld >= (long)(H + 2 * Hkv) * hd && al16(qkv) && al16(kq) && al16(vq),
                 "kv8_rope_append: rows of ld=%ld must be 16-byte multiples that hold q|k|v, code planes 16-byte aligned", ld);
    AV_CHECK_ARG(Tmax > 0 && pos >= 0 && (pos_dev || pos < Tmax), "kv8_rope_append: pos=%d outside the cache (Tmax=%d)", pos, Tmax);
    Kv8RopeArgs a = {(bf16*)qkv, ld, B, H, Hkv, hd, rotate ? 1 : 0, rope, Kv8Planes{(uint8_t*)kq, (uint8_t*)ke, (uint8_t*)vq, (uint8_t*)ve}, Tmax, pos, pos_dev};
    const long per = (rotate ? (long)H * (hd >> 4) : 0) + (long)Hkv * (hd >> 6) + (long)Hkv * (hd >> 5);
    const long total = per * B;
    AV_CHECK_ARG(total < (1L << 30), "kv8_rope_append: too many rows");
    hipLaunchKernelGGL(kv8_rope_append_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

// both planes through kv_gather_rows as rows of bytes (its bf16 form with half as many elements): code rows of dkv bytes, exponent rows of dkv/32
int av_kv8_gather_rows(const void* k_src, const void* v_src, int src_rows, long src_T, void* k_dst, void* v_dst, int dst_rows, long dst_T, int layers,
                       int dkv, const int32_t* parent, int t0, int t1, hipStream_t st) {
    AV_CHECK_ARG(k_src && v_src && k_dst && v_dst && layers > 0 && src_rows > 0 && dst_rows > 0 && src_T > 0 && dst_T > 0, "kv8_gather_rows: null/empty");
    AV_CHECK_ARG(dkv > 0 && dkv % 64 == 0, "kv8_gather_rows: dkv=%d must be a multiple of 64", dkv);
    const size_t cs = (size_t)layers * src_rows * src_T * dkv, cd = (size_t)layers * dst_rows * dst_T * dkv;
    AV_TRY(av_kv_gather_rows(k_src, v_src, src_rows, src_T, k_dst, v_dst, dst_rows, dst_T, layers, dkv / 2, parent, t0, t1, AV_BF16, st));
    return av_kv_gather_rows((const char*)k_src + cs, (const char*)v_src + cs, src_rows, src_T, (char*)k_dst + cd, (char*)v_dst + cd, dst_rows, dst_T, layers,
                             dkv / 64, parent, t0, t1, AV_BF16, st);
}

extern "C" int avllm_kv8_append(const void* k, const void* v, int64_t ld, void* k_codes, void* k_exps, void* v_codes, void* v_exps, int32_t B, int32_t T,
                                int32_t pos0, int32_t Tmax, int32_t dkv, void* stream) {
    return av_kv8_append(k, v, ld, k_codes, k_exps, v_codes, v_exps, B, T, pos0, Tmax, dkv, (hipStream_t)stream);
}
extern "C" int avllm_kv8_rope_append(void* qkv, int64_t ld, int32_t B, int32_t heads, int32_t kv_heads, int32_t hd, const float* rope, int32_t rotate,
                                     void* k_codes, void* k_exps, void* v_codes, void* v_exps, int32_t Tmax, int32_t pos, const int32_t* pos_dev, void* stream) {
    return av_kv8_rope_append(qkv, ld, B, heads, kv_heads, hd, rope, rotate, k_codes, k_exps, v_codes, v_exps, Tmax, pos, pos_dev, (hipStream_t)stream);
}
extern "C" int avllm_kv8_gather_rows(const void* k_src, const void* v_src, int32_t src_rows, int64_t src_T, void* k_dst, void* v_dst, int32_t dst_rows,
                                     int64_t dst_T, int32_t layers, int32_t dkv, const int32_t* parent, int32_t t0, int32_t t1, void* stream) {
    return av_kv8_gather_rows(k_src, v_src, src_rows, src_T, k_dst, v_dst, dst_rows, dst_T, layers, dkv, parent, t0, t1, (hipStream_t)stream);
}
