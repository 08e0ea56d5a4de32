// Device pieces shared by the MFMA attention kernels of attention.hip and attention_bwd.hip (32x32x16 geometry: one wave owns 32 rows, the row
// index lives on the MFMA lane).  Every piece is a __device__ __forceinline__ function or template and none branches on its caller.
// attn_fwd_short (16x16x32 geometry, K and V images of different row counts) takes the LDS typedefs only.  attn_fwd_mfma stages K and V as a
// PAIR (one predicate per chunk for both tensors) in a loop of its own: as a function here, in every form tried, that loop costs the head_dim 64
// kernels a register or more, and two load_rows calls double the exec-mask branches of its key loop (profiles/r14_attention_refactor_isa.txt).
#pragma once
#include "common.h"

namespace avt {

typedef __attribute__((address_space(3))) short4v* lds_s4_ptr;
typedef __attribute__((ext_vector_type(8))) short short8v;

// row of a 32x32 MFMA accumulator that register `reg` of a lane in half `half` (lane >> 5) holds
__device__ __forceinline__ int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// A operand = X^T fragment for the 32x32x16 MFMA: rows = 32 columns of the LDS tile starting at col0, k = 16 tile rows
// starting at row0 (permuted order matching an accumulator-as-B operand: element j <-> row 8(j>>2)+4half+(j&3))
__device__ __forceinline__ bf16x8 tr_frag(const char* img, int stride, int row0, int col0, int lane) {
    const int g = lane >> 4, i16 = lane & 15, half = lane >> 5;
    const char* a0 = img + (row0 + 4 * half + (i16 >> 2)) * stride + (col0 + 16 * (g & 1) + 4 * (i16 & 3)) * 2;
    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)(a0));
    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)(a0 + 8 * stride));
    const short8v both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, both);
}

// Tiles go global -> registers -> LDS, so that the loads of a tile can be issued before the barrier that frees its LDS image and their latency
// runs under other work.  ROWS rows of HD bf16 are spread over the NT threads of the workgroup as 16-byte chunks; rows past rows_max are zero.
template <int HD, int NT, int ROWS> struct RowRegs { u32x4 v[(ROWS * (HD / 8) + NT - 1) / NT]; };

template <int HD, int NT, int ROWS>
__device__ __forceinline__ void load_rows(RowRegs<HD, NT, ROWS>& r, const bf16* __restrict__ src, long ld, int row0, int rows_max, int tid) {
    constexpr int CPR = HD / 8, N = (ROWS * CPR + NT - 1) / NT;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int c = tid + i * NT, row = c / CPR, ch = c % CPR;
        r.v[i] = (u32x4){0u, 0u, 0u, 0u};
        if (c < ROWS * CPR && row0 + row < rows_max) r.v[i] = *(const u32x4*)(src + (long)(row0 + row) * ld + ch * 8);
    }
}
template <int HD, int NT, int ROWS>
__device__ __forceinline__ void store_rows(const RowRegs<HD, NT, ROWS>& r, char* img_a, int stride_a, char* img_b, int stride_b, int tid) {
    constexpr int CPR = HD / 8, N = (ROWS * CPR + NT - 1) / NT;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int c = tid + i * NT, row = c / CPR, ch = c % CPR;
        if (c < ROWS * CPR) {
            if (img_a) *(u32x4*)(img_a + row * stride_a + ch * 16) = r.v[i];
            if (img_b) *(u32x4*)(img_b + row * stride_b + ch * 16) = r.v[i];
        }
    }
}

// One row of a transposed 32 x HD result held in the MFMA output layout (lane = row, registers [d][4 g4 + i] = element 32 d + 8 g4 + 4 half + i),
// times mul, rounded once: the epilogue of the forward (mul = 1 / l) and of dq (mul = 1).
template <int HD>
__device__ __forceinline__ void store_acc_rows(bf16* row, const f32x16 (&acc)[HD / 32], int half, float mul) {
#pragma unroll
    for (int d = 0; d < HD / 32; ++d)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            float vals[4] = {acc[d][4 * g4] * mul, acc[d][4 * g4 + 1] * mul, acc[d][4 * g4 + 2] * mul, acc[d][4 * g4 + 3] * mul};
            store_f<4>(row + 32 * d + 8 * g4 + 4 * half, vals);
        }
}

}  // namespace avt
