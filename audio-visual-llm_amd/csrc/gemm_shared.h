// Pieces shared by the GEMM kernels of gemm.hip, gemm_dp.hip, fp8_fast.hip and fp8.hip; DESIGN.md "Which GEMM kernel a call gets" lists which
// kernel uses which.  Everything is a __device__ __forceinline__ function or template, or a macro around one inline-asm statement.  A piece is
// shared only where the hand-scheduled kernels that use it (gemm_bf16_w / _wp / _dp, gemm_f8_wp) keep the instruction stream they had with a
// private copy (tools/kernel_isa_diff.py, profiles/r10_gemm_dedup_isa.txt): the compiler simplifies a helper on its own BEFORE inlining it,
// and what it can already fold there changes branch layout and register allocation of everything around the call.
#pragma once
#include "common.h"
#include <utility>
#include <type_traits>

// cache-policy bits of the operand DMA of the 4-wave kernels (experiment: tools/gemm_dma_policy.sh builds one library per policy); default none
#ifndef AVLLM_DMA_POLICY
#define AVLLM_DMA_POLICY ""
#endif
// The instructions of the hand-written K loops (gemm_bf16_w / wp / dp, gemm_f8_wp): a fragment read, one operand DMA (LDS address in m0, SGPR base
// + 32-bit VGPR offset), and the "every accumulator of row I is an in/out operand" statement that keeps compiler-generated readers behind it.
#define AV_W_RD(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#define AV_W_LD(voff, base, m0v) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" AVLLM_DMA_POLICY :: "s"(m0v), "v"(voff), "s"(base) : "memory")
#define AV_W_PIN4(I) asm volatile("" : "+a"(acc[I][0]), "+a"(acc[I][1]), "+a"(acc[I][2]), "+a"(acc[I][3]))
#define AV_W_PIN8(I) asm volatile("" : "+a"(acc[I][0]), "+a"(acc[I][1]), "+a"(acc[I][2]), "+a"(acc[I][3]), "+a"(acc[I][4]), "+a"(acc[I][5]), "+a"(acc[I][6]), "+a"(acc[I][7]))
// B-operand (weight) fragment j of a wave of the persistent kernels reads LDS rows 32 (j >> 1) + 4 (j & 1) + 8 (fr >> 2) + (fr & 3) of its half: MFMA
// tiles 2p and 2p+1 then hold, in lane (fr, fq), output columns 32p + 8fq + {0..3} and + {4..7} of row fr -- one 16-byte bf16 chunk per lane and tile
// pair, stored straight from the accumulators (no LDS transpose in the epilogue).  Byte offset of fragment j from the lane's base row, for LDS rows
// of `pitch` bytes (128: gemm_bf16_wp, gemm_f8_wp; 64: gemm_bf16_dp):
#define WP_BOFF(j, pitch) ((((j) >> 1) * 32 + ((j) & 1) * 4) * (pitch))

namespace avg {

template <int I, int N, class F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<I + 1, N>(f); }
}

// f(std::integral_constant<int, ACT>{}) for the runtime activation: one instantiation of f's body per activation, chosen by a uniform branch.
// Used by the LDS-staged epilogues of gemm_bf16_h / _w.  The persistent kernels spell the same ladder out at the end of their choice among the
// epilogue forms (and gemm_f8_wp for its quantised output): as a function its compare chain is folded into a switch before it is inlined, and
// their instruction streams change.
template <class F> __device__ __forceinline__ void with_act(int act, F&& f) {
    if (act == AV_ACT_NONE) f(std::integral_constant<int, AV_ACT_NONE>{});
    else if (act == AV_ACT_GELU) f(std::integral_constant<int, AV_ACT_GELU>{});
    else if (act == AV_ACT_QUICK_GELU) f(std::integral_constant<int, AV_ACT_QUICK_GELU>{});
    else f(std::integral_constant<int, AV_ACT_SILU>{});
}

// Lean item of the LDS-staged epilogue for the common case (bf16 output, alpha = 1, no dropout, no row remap, plain residual, tile fully
// inside the matrix): the general epilogue_store8 spends most of its instructions on 64-bit index arithmetic and on uniform branches
// around features these calls do not use.  lo/hi = the two fp32 LDS chunks of this item, b = the thread's bias (zeros without one).
template <int ACT>
__device__ __forceinline__ void epilogue_fast8(const f32x4 lo, const f32x4 hi, const float (&b)[8], bool has_b, const bf16* rp, bf16* cp) {      // rp may alias cp (in-place residual)
    float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    if (has_b) {                                                   // uniform
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] += b[i];
    }
    if constexpr (ACT != AV_ACT_NONE) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = act_apply_fast(v[i], ACT);
    }
    if (rp) {
        const bf16x8 r = *(const bf16x8*)rp;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] += (float)r[i];
    }
    store_f<8>(cp, v);
}

// XCD-aware remap: blocks b and b+8 share an XCD (round-robin dispatch); give each XCD a contiguous
// range of logical tile ids.  Bijective for any grid size (cdna guide §5, "XCD swizzle must be bijective").
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (bid >> 3);
}

// gw > 0 (tall shapes, tiles_m > 32): COLUMN GROUPS of gw tile columns, ids run row-major inside a group (tn fastest) and group after group.
// With one contiguous id range per XCD (xcd_remap) an XCD then works inside ONE group for most of the launch: its gw weight panels
// (gw x 256 x K x 2 bytes: 1.2 - 1.6 MB at K = 768) stay L2-resident and each activation panel is fetched once per group and shared by the gw
// CUs that hold its tiles at that moment.  Plain row-major order over all tiles_n columns (gw = 0) cycles the whole weight matrix (4.7 MB for the
// CLIP fc1 > the 4 MiB L2) through every XCD: profiles/r03_pmc_gemm_shapes.txt measured 8.8x (fc1) / 5.3x (qkv) the algorithmic read bytes.
__device__ __forceinline__ void tile_coords(int id, int tiles_m, int tiles_n, int& tm, int& tn, int blocked = 0, int gw = 0) {
    if (gw > 0 && tiles_m > 32 && tiles_n > gw) {
        const int per_group = gw * tiles_m, ngf = tiles_n / gw, full = ngf * per_group;
        if (id < full) {
            const int grp = id / per_group, in = id - grp * per_group;
            tm = in / gw; tn = grp * gw + (in - tm * gw);
        } else {
            const int r = id - full, rem = tiles_n - ngf * gw;
            tm = r / rem; tn = ngf * gw + (r - tm * rem);
        }
        return;
    }
    if (blocked && tiles_m <= 32 && tiles_m % 8 == 0) {
        // 8 x 4 blocks of tiles per 32 consecutive ids (an XCD's share of a round): half the activation panel and four weight panels per XCD
        // and round instead of the whole activation panel and two weight panels -- a third fewer bytes into each L2.  Measured on the
        // Llama shapes (M = 4096): gate|up 604 -> 578 us, d(gate,up) 527 -> 503, fused qkv 341 -> 329, d(lm_head) 734 -> 709; one-round
        // shapes unchanged.  AVLLM_GEMM_DBG bit 2 restores the row-major order.
        const int full = (tiles_n / 4) * 4 * tiles_m;
        if (id < full) {
            const int per_group = 4 * tiles_m, grp = id / per_group, in = id - grp * per_group;
            const int c = in >> 5, w = in & 31;
            tm = c * 8 + (w & 7);
            tn = grp * 4 + (w >> 3);
            return;
        }
        const int r = id - full;
        tm = r % tiles_m; tn = (tiles_n / 4) * 4 + r / tiles_m;
        return;
    }
    if (tiles_m <= 32) { tm = id % tiles_m; tn = id / tiles_m; }      // weights streamed once, all row tiles adjacent
    else               { tn = id % tiles_n; tm = id / tiles_n; }      // activations streamed once
}

// ------------------------------------------------------------------------------------------ compiler-scheduled kernels (gemm_bf16 / _l / _h / _hp)
// one wave-instruction of operand staging: 8 rows x 128 B, global -> LDS rows [group*8, group*8+8); 16-byte chunk index ^ (row & 7) on the source
__device__ __forceinline__ void stage_rows8(const bf16* __restrict__ base, long ld, int row0, int rows_max, int k0, char* lds,
                                            int group, int lane) {
    const int rsub = lane >> 3;
    int gr = row0 + group * 8 + rsub;
    gr = gr < rows_max ? gr : rows_max - 1;          // clamp: rows past the edge are never stored
    const bf16* src = base + (long)gr * ld + k0 + (((lane & 7) ^ rsub) << 3);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)(lds + group * 1024), 16, 0, 0);      // wave-uniform base; hardware adds lane*16
}

// One 64-wide K-tile of a 64x64 wave tile at rows wm*64 of the activation image and wn*64 of the weight image (128-byte rows, swizzled as
// staged): per k-half 8 ds_read_b128 and 4x4 MFMA 16x16x32, the weight fragment as the A operand (acc = W_frag x X_frag).
__device__ __forceinline__ void wave_tile_64x64(f32x4 (&acc)[4][4], const char* a_lds, const char* b_lds, int wm, int wn, int fr, int fq) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        bf16x8 xa[4], wb[4];
        const int chunk = ks * 4 + fq;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = wm * 64 + i * 16 + fr;
            xa[i] = *(const bf16x8*)(a_lds + r * 128 + ((chunk ^ (r & 7)) << 4));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = wn * 64 + j * 16 + fr;
            wb[j] = *(const bf16x8*)(b_lds + r * 128 + ((chunk ^ (r & 7)) << 4));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[j], xa[i], acc[i][j], 0, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------ K-step table of the 4-wave kernels (gemm_bf16_w / _wp)
// fragment j of the weight operand, bytes from the lane's base row: rows 16 j (one-shot kernel) or the column-interleaved order of WP_BOFF
struct BoffLinear { static constexpr int of(int j) { return j * 2048; } };
struct BoffPaired { static constexpr int of(int j) { return WP_BOFF(j, 128); } };

// Slot N of a 64-wide K-step = 128 MFMAs of a 128x128 wave quadrant: N = 64 h + n, MFMA n of k-half h = accumulator (n >> 3, n & 7), then whatever
// else the slot carries: the fragments of BOTH k-halves of both operands sit in registers, so an operand's half of the current LDS buffer is dead
// after 8 ds_reads per wave and is refilled in place by the DMA with the data of K-step t+2.  Three barriers and three full lgkmcnt waits per 128
// MFMAs, every ds_read issued >= 10 MFMAs before its wait, loads one per 2-3 MFMAs.
// la1/lb1: this lane's k-half-1 fragment address in the CURRENT buffer; la0/lb0: k-half 0 in the OTHER buffer (next K-step).
// MODE 0: any K-step but a tile's first; 1: a tile's first K-step (accumulators start from 0); 2: the same right after the epilogue of a
// tile that lay fully inside the matrix.  vmcnt counts loads and stores together in issue order, so the counted wait of the K-step would
// also wait for the 32 epilogue stores issued just before it (their write acknowledgements take several microseconds when the whole
// grid stores at once); mode 2 allows exactly those 32 to stay in flight: everything OLDER (the K-step's operands) has still landed.
template <int N, int MODE, class BOFF>
__device__ __forceinline__ void wgemm_step(f32x4 (&acc)[8][8], bf16x8 (&FA)[2][8], bf16x8 (&FB)[2][8], int la1, int la0, int lb1, int lb0,
                                           const unsigned (&vA)[8], const unsigned (&vB)[8], const bf16* pA, const bf16* pB, int m0A, int m0B) {
    constexpr int h = N >> 6, n = N & 63, I = n >> 3, J = n & 7;
    if constexpr (MODE != 0 && h == 0) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=a"(acc[I][J]) : "v"(FB[h][J]), "v"(FA[h][I]));
    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[I][J]) : "v"(FB[h][J]), "v"(FA[h][I]));
    if constexpr (h == 0) {
        if constexpr (n < 16 && (n & 1)) AV_W_RD(FB[1][n >> 1], lb1, BOFF::of(n >> 1));
        if constexpr (n == 20) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (n == 21) __builtin_amdgcn_s_barrier();                          // every wave has read all of B(cur)
        if constexpr (n >= 22 && n < 38 && !(n & 1)) AV_W_LD(vB[(n - 22) >> 1], pB, m0B + ((n - 22) >> 1) * 1024);
        if constexpr (n >= 23 && n < 39 && (n & 1)) AV_W_RD(FA[1][(n - 23) >> 1], la1, ((n - 23) >> 1) * 2048);
        if constexpr (n == 50) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (n == 51) __builtin_amdgcn_s_barrier();                          // ... and all of A(cur)
        if constexpr (n == 52 || n == 55 || n == 58 || n == 61) AV_W_LD(vA[(n - 52) / 3], pA, m0A + ((n - 52) / 3) * 1024);
    } else {
        if constexpr (n == 0) AV_W_LD(vA[4], pA, m0A + 4 * 1024);
        // 13 loads of this step issued so far: all older ones have landed
        if constexpr (n == 26) { if constexpr (MODE == 2) asm volatile("s_waitcnt vmcnt(45)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); }
        if constexpr (n == 27) __builtin_amdgcn_s_barrier();                          // the other buffer is complete for every wave
        if constexpr (n >= 28 && n < 36) AV_W_RD(FB[0][n - 28], lb0, BOFF::of(n - 28));
        if constexpr (n >= 37 && n < 53 && (n & 1)) AV_W_RD(FA[0][(n - 37) >> 1], la0, ((n - 37) >> 1) * 2048);
        if constexpr (n == 32 || n == 40 || n == 48) AV_W_LD(vA[5 + (n - 32) / 8], pA, m0A + (5 + (n - 32) / 8) * 1024);
        if constexpr (n == 62) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

template <int MODE, class BOFF, int... Ns>
__device__ __forceinline__ void wgemm_kstep(std::integer_sequence<int, Ns...>, f32x4 (&acc)[8][8], bf16x8 (&FA)[2][8], bf16x8 (&FB)[2][8], int la1, int la0,
                                            int lb1, int lb0, const unsigned (&vA)[8], const unsigned (&vB)[8], const bf16* pA, const bf16* pB, int m0A, int m0B) {
    (wgemm_step<Ns, MODE, BOFF>(acc, FA, FB, la1, la0, lb1, lb0, vA, vB, pA, pB, m0A, m0B), ...);
}

// ------------------------------------------------------------------------------------------ accumulator epilogue of the persistent kernels
// (gemm_bf16_wp <P = 4, RD = WP_RES_DEPTH>, gemm_bf16_dp <2, 7>, gemm_f8_wp <4, 1>)
// Epilogue straight from the accumulators of a 128-row wave tile with the column-interleaved weight fragments (WP_BOFF): lane (fr, fq) holds, for
// row block i and column pair p < P, the 8 consecutive output columns 32p + 8fq .. +7 of row 16i + fr (acc[i][2p] = the first four, acc[i][2p+1]
// = the last four): bias / activation / residual on the fp32 values, one rounding, one 16-byte store per pair; a store instruction covers 16
// rows x 64 contiguous bytes.  b = the lane's bias values (zeros without one: the bias cannot ride in the accumulators' initial value, an MFMA's C
// and D operands share one register-file bit, and D is an AGPR); cp0 / rp0 = output / residual at the lane's first row m0 and column n; item
// (i, p) is 16 i rows down and 32 p columns right: uniform (scalar) multiples of the row strides ldc / ldr.
// Every form "redefines" the accumulators for the compiler chunk by chunk: without it every form's accumulator reads are hoisted above the
// kernel's branch between the forms as common subexpressions -- 256 live registers (gemm_f8_wp: 57 spilled VGPRs, 460 scratch accesses around
// the epilogue; gemm_bf16_wp: ~130 spills).
// The bias preload and the choice among the forms stay in the kernels, and every argument is taken BY REFERENCE: helpers are simplified on their
// own before they are inlined, and anything a helper could already fold there (by-value arguments, a compare chain on the activation) changed
// the branch layout and the register allocation of the hand-scheduled kernels around it (tools/kernel_isa_diff.py).

// edge tiles (and activation + residual, which no model call makes): per-chunk bounds tests; dbg bit 0 = experiment, no stores
template <int P, int ACT>
__device__ __forceinline__ void acc_store_general(f32x4 (&acc)[8][2 * P], const float (&b)[P][8], const bool& has_b, bf16* const& cp0, const bf16* const& rp0,
                                                  const long& ldc, const long& ldr, const int& m0, const int& n, const int& M, const int& N, const int& dbg) {
#pragma clang loop unroll(full)
    for (int i = 0; i < 8; ++i) {
        const bool mrow = m0 + i * 16 < M;
#pragma clang loop unroll(full)
        for (int p = 0; p < P; ++p) {
            asm volatile("" : "+a"(acc[i][2 * p]), "+a"(acc[i][2 * p + 1]));
            if (mrow && n + 32 * p < N && !(dbg & 1))
                epilogue_fast8<ACT>(acc[i][2 * p], acc[i][2 * p + 1], b[p], has_b, rp0 ? rp0 + (i * 16) * ldr + 32 * p : nullptr, cp0 + (i * 16) * ldc + 32 * p);
        }
    }
}

// full tile, no residual: 8 accumulator reads, 8 bias adds (only in the instantiation with a bias), the activation, 4 packed converts and
// one 16-byte store per chunk -- no bounds test, no select, no branch (the general form above spends ~40 instructions per chunk:
// tools/gemm_stamps.py measured the epilogue at a quarter of a K = 768 tile).
// sp: store policy, experiment builds of gemm.hip only (sp.store(...) = true: the policy stored the chunk itself).
struct PlainStores { static constexpr bool on = false; };
template <int P, int ACT, bool HASB, class SP = PlainStores>
__device__ __forceinline__ void acc_store_full(f32x4 (&acc)[8][2 * P], const float (&b)[P][8], bf16* const& cp0, const long& ldc, SP&& sp = SP{}) {
#pragma clang loop unroll(full)
    for (int i = 0; i < 8; ++i) {
        bf16* const cpi = cp0 + (long)(i * 16) * ldc;
#pragma clang loop unroll(full)
        for (int p = 0; p < P; ++p) {
            asm volatile("" : "+a"(acc[i][2 * p]), "+a"(acc[i][2 * p + 1]));
            const f32x4 lo = acc[i][2 * p], hi = acc[i][2 * p + 1];
            float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            if constexpr (HASB) {
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] += b[p][c];
            }
            if constexpr (ACT != AV_ACT_NONE) {
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] = act_apply_fast(v[c], ACT);
            }
            if constexpr (std::remove_reference_t<SP>::on) {
                if (sp.store(cpi + 32 * p, v, i == 7 && p == P - 1)) continue;
            }
            store_f<8>(cpi + 32 * p, v);
        }
    }
}

// full tile + residual (out-projection, fc2, o, down, gradient sums): the residual chunks of RD row blocks ahead of the one being stored (7 = ALL
// 8 P chunks of the lane in one burst) are requested into registers the operand fragments occupy during the K loop, then consumed in issue
// order.  gemm_bf16_wp / _dp re-read the next tile's fragments after the epilogue, so all of them are dead here and the tile pays one memory
// latency instead of one per row block (tools/gemm_stamps.py: 12 us of a 29 us out-projection tile with the one-row-block-ahead form);
// gemm_f8_wp carries the next tile's 128 fragment registers through the epilogue and has room for one row block ahead only.  A load may alias
// a later store (in-place residual): every load is issued before the first store to its bytes, and a lane only ever reads the bytes it writes
// itself.  Younger operations behind chunk (i, p)'s load at its wait: the P - 1 other loads of its own asm statement, P per later row block
// in flight, P stores per row block stored since the loads were issued: (P - 1) + P ahead + P behind; with the whole tile in flight that is
// 8 P - 1 whatever (i, p): one constant vmcnt.  asm loads + explicit waits because compiler-visible loads consumed later leave the wait-count
// pass with pending state that reaches the K loop as vmcnt(0) per K-step.
template <int P, int RD, bool HASB>
__device__ __forceinline__ void acc_store_full_res(f32x4 (&acc)[8][2 * P], const float (&b)[P][8], bf16* const& cp0, const bf16* const& rp0, const long& ldc,
                                                   const long& ldr) {
    static_assert(P == 2 || P == 4, "the residual loads are written for 2 or 4 chunks per row block");
    u32x4 rr[RD + 1][P];
    auto fetch = [&](int i) __attribute__((always_inline)) {               // i: a constant once inlined
        const int s = i % (RD + 1);
        const bf16* rp = rp0 + (long)(i * 16) * ldr;
        if constexpr (P == 4)
            asm volatile("global_load_dwordx4 %0, %4, off\n\tglobal_load_dwordx4 %1, %4, off offset:64\n\t"
                         "global_load_dwordx4 %2, %4, off offset:128\n\tglobal_load_dwordx4 %3, %4, off offset:192"
                         : "=&v"(rr[s][0]), "=&v"(rr[s][1]), "=&v"(rr[s][2]), "=&v"(rr[s][3]) : "v"(rp) : "memory");
        else
            asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %2, off offset:64" : "=&v"(rr[s][0]), "=&v"(rr[s][1]) : "v"(rp) : "memory");
    };
#pragma clang loop unroll(full)
    for (int i = 0; i < RD && i < 8; ++i) fetch(i);
    static_for<0, 8>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        if constexpr (i + RD < 8) fetch(i + RD);
        bf16* const cpi = cp0 + (long)(i * 16) * ldc;
        constexpr int ahead = (i + RD < 8 ? i + RD : 7) - i, behind = RD < i ? RD : i, nw = (P - 1) + P * ahead + P * behind;
        static_for<0, P>([&](auto pc) __attribute__((always_inline)) {
            constexpr int p = decltype(pc)::value;
            u32x4& x = rr[i % (RD + 1)][p];
            asm volatile("s_waitcnt vmcnt(%1)" : "+v"(x) : "n"(nw) : "memory");
            const bf16x8 r = __builtin_bit_cast(bf16x8, x);
            asm volatile("" : "+a"(acc[i][2 * p]), "+a"(acc[i][2 * p + 1]));
            const f32x4 lo = acc[i][2 * p], hi = acc[i][2 * p + 1];
            float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            if constexpr (HASB) {
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] += b[p][c];
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] += (float)r[c];
            store_f<8>(cpi + 32 * p, v);
        });
    });
}

}  // namespace avg
