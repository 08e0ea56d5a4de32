// OCP MXFP4 weight images for the token step's fp4 weight form (decode.hip, dec_proj_f4_kernel): e2m1 elements, one E8M0 scale per 32
// consecutive K elements.  Weight-only and load-time: this file holds the quantiser alone; the codes are consumed in registers by
// v_cvt_scalef32_pk_bf16_fp4 in the decode projections.
//
// Formats
//   q     uint8 [R, K/2] row-major: byte i of a row = code of element 2i in bits 3:0, code of element 2i+1 in bits 7:4 (the order in which
//         v_cvt_scalef32_pk_bf16_fp4 delivers a byte's two results).  code = sign << 3 | index into {0, 0.5, 1, 1.5, 2, 3, 4, 6}
//   exps  uint8 [R, K/32] row-major, E8M0 biased by 127 (the "layout 2" of the fp8 images)
// Rule (OCP MX v1.0 §6.3 with emax = 2 of e2m1): e = floor(log2(amax)) - 2 clamped to [-127, 127]; elements = RNE(x * 2^-e) saturated to +-6.
#include "common.h"
#include "avllm_internal.h"
#include "mx.h"

namespace {

// |x| * 2^-e -> e2m1 index, round to nearest, ties to the even code (0.25 -> 0, 0.75 -> 1.0, 1.25 -> 1.0, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4)
__device__ __forceinline__ uint32_t e2m1_index(float a) {
    return (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) + (uint32_t)(a > 2.5f) + (uint32_t)(a >= 3.5f) +
           (uint32_t)(a > 5.0f);
}

// one thread = one 32-element block: 16 bytes of codes + one exponent byte
template <typename T>
__global__ __launch_bounds__(256) void mx4_quant_kernel(const T* __restrict__ x, long ldx, int R, int K, uint8_t* __restrict__ q, long ldq,
                                                        uint8_t* __restrict__ exps) {
    const int nkb = K >> 5;
    const long total = (long)R * nkb;
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int kb = (int)(idx % nkb);
        const long row = idx / nkb;
        float v[32];
        mx_load32(x + row * ldx + kb * 32, v);
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 32; ++j) amax = fmaxf(amax, fabsf(v[j]));
        const int e = mx_block_exp<MX_EMAX_E2M1>(amax);
        const float invs = mx_inv_scale(e);
        uint32_t pk[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t wd = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float f = v[8 * j + c];
                wd |= (e2m1_index(fabsf(f) * invs) | (f < 0.f ? 8u : 0u)) << (4 * c);
            }
            pk[j] = wd;
        }
        *(u32x4*)(q + row * ldq + kb * 16) = (u32x4){pk[0], pk[1], pk[2], pk[3]};
        exps[row * nkb + kb] = (uint8_t)mx_exp_byte(e);
    }
}

}  // namespace

extern "C" int avllm_mx4_quantize(const void* x, int64_t ldx, int32_t R, int32_t K, void* q, int64_t ldq, void* exps, int32_t dtype, void* stream) {
    AV_CHECK_ARG(x && q && exps && R > 0 && K > 0, "mx4_quantize: null/empty");
    AV_CHECK_ARG(dtype == AV_BF16 || dtype == AV_F32, "mx4_quantize: dtype %d", dtype);
    AV_CHECK_ARG(K % 32 == 0 && ldx % 8 == 0 && ldx >= K && ldq % 16 == 0 && ldq >= K / 2 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)x & 15) == 0,
                 "mx4_quantize: K=%d must be a multiple of 32, rows 16-byte aligned (ldx=%ld, ldq=%ld bytes)", K, (long)ldx, (long)ldq);
    const long total = (long)R * (K / 32);
    long blocks = (total + 255) / 256;
    blocks = blocks > 65536 ? 65536 : blocks;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == AV_BF16) hipLaunchKernelGGL((mx4_quant_kernel<bf16>), dim3(blocks), dim3(256), 0, st, (const bf16*)x, ldx, R, K, (uint8_t*)q, ldq, (uint8_t*)exps);
    else hipLaunchKernelGGL((mx4_quant_kernel<float>), dim3(blocks), dim3(256), 0, st, (const float*)x, ldx, R, K, (uint8_t*)q, ldq, (uint8_t*)exps);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
