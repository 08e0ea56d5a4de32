// The OCP MX block rule (MX v1.0 §6.3), once for the device: 32 consecutive elements share one E8M0 exponent, stored biased by 127.
//   e = floor(log2 amax) - emax of the element format (e4m3: 8, e2m1: 2), clamped to [-127, 127]; amax == 0 or subnormal -> -127 (byte 0)
//   elements = RNE(x * 2^-e), saturated to the format's largest magnitude (e4m3: +-448)
// The host statement of the same rule is oracle/mxfp8.py.  The quantisers and readers of MX data in csrc/ are made of these pieces (one epilogue,
// in fp8_fast.hip, writes the rule out and says why); a site that finds amax across lanes keeps its own shuffles and stores and takes the rule
// from here.
#pragma once
#include "common.h"

constexpr int MX_EMAX_E4M3 = 8, MX_EMAX_E2M1 = 2;

// ---- encode
// block exponent: floor(log2 amax) read off the exponent field
template <int EMAX> __device__ __forceinline__ int mx_block_exp(float amax) {
    const int e = (int)((__float_as_uint(amax) >> 23) & 0xff) - 127 - EMAX;
    return e < -127 ? -127 : (e > 127 ? 127 : e);
}
// 2^-e: e <= 128 - emax for any amax, so the exponent field stays >= 1
__device__ __forceinline__ float mx_inv_scale(int e) { return __uint_as_float((uint32_t)(127 - e) << 23); }
// the stored byte, as the value a caller shifts into a scale word or narrows to uint8_t
__device__ __forceinline__ uint32_t mx_exp_byte(int e) { return (uint32_t)(e + 127); }
// N floats (a multiple of 4) at v times invs, saturated, as N/4 dwords of e4m3 codes at pk (element i in byte i & 3 of dword i / 4).  In place:
// v is left holding the saturated values (through a copy the attention epilogue's instructions come out in another order)
template <int N> __device__ __forceinline__ void mx_pack_e4m3(float* v, float invs, uint32_t* pk) {
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = fminf(fmaxf(v[c] * invs, -448.f), 448.f);
#pragma unroll
    for (int j = 0; j < N / 4; ++j) {
        int r = 0;
        r = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * j], v[4 * j + 1], r, false);
        r = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * j + 2], v[4 * j + 3], r, true);
        pk[j] = (uint32_t)r;
    }
}

// ---- a whole block owned by one thread
template <typename T> __device__ __forceinline__ void mx_load32(const T* p, float (&v)[32]) {
#pragma unroll
    for (int c = 0; c < 32; c += 8) {
        float t8[8];
        load_f<8>(p + c, t8);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[c + j] = t8[j];
    }
}
// 32 values -> 32 e4m3 codes in pk; returns the block exponent
__device__ __forceinline__ int mx_block32_quant(const float (&v)[32], uint32_t (&pk)[8]) {
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) amax = fmaxf(amax, fabsf(v[j]));
    const int e = mx_block_exp<MX_EMAX_E4M3>(amax);
    const float invs = mx_inv_scale(e);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float a[4] = {v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
        mx_pack_e4m3<4>(a, invs, pk + j);
    }
    return e;
}
// the same, stored: codes at qp (16-byte aligned), exponent byte at ep
__device__ __forceinline__ void mx_block32_store(const float (&v)[32], uint8_t* qp, uint8_t* ep) {
    uint32_t pk[8];
    const int e = mx_block32_quant(v, pk);
    *(u32x4*)qp = (u32x4){pk[0], pk[1], pk[2], pk[3]};
    *(u32x4*)(qp + 16) = (u32x4){pk[4], pk[5], pk[6], pk[7]};
    *ep = (uint8_t)mx_exp_byte(e);
}

// ---- decode
// exponent byte -> 2^(e - 127); byte 0 (an all-zero block) -> 0
__device__ __forceinline__ float mx_e8m0(unsigned byte) { return __uint_as_float(byte << 23); }
// 16 e4m3 codes -> fp32 (exact), unscaled
__device__ __forceinline__ void mx_codes16(const u32x4 c, float (&o)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], true);
        o[4 * i] = lo[0]; o[4 * i + 1] = lo[1]; o[4 * i + 2] = hi[0]; o[4 * i + 3] = hi[1];
    }
}
