// Greedy-decode token step (clip_whisper_model.py:1337-1340 -> GenerationMixin greedy search, one new token per sequence on a KV cache):
// every frozen weight is streamed from HBM exactly once per step whatever the batch, so the step is a chain of
// HBM-bound weight streams and its floor is weight bytes / HBM rate.  Round 1 ran 10 launches per decoder layer (norm, q|k|v, RoPE,
// cache append, attention, o, norm, gate|up, SwiGLU, down), five of them on the ~5 us launch floor; here a layer is 5 launches, and this
// file is dec_proj, four of the five (the attention is attention_decode.hip):
//
//   dec_proj<NORM, qkv>      RMSNorm folded into the A operand, q|k|v projection, RoPE on q/k in the accumulators, k/v written
//                            straight into the cache row of this position
//   attn_decode1             one pass over the cache rows (online softmax), up to 16 waves per (sequence, head)
//   dec_proj<plain + R>      o projection + residual
//   dec_proj<NORM, SwiGLU>   RMSNorm folded in, gate|up projection, silu(gate)*up in the epilogue
//   dec_proj<plain + R>      down projection + residual
//
// A model whose q and k heads are normalised before RoPE (Qwen3) runs 6: the q|k|v projection leaves its columns raw (raw_qkv below) and one
// avllm_qk_norm_rope launch (qk_norm.hip) normalises, rotates and writes the cache row before attn_decode1.
//
// dec_proj: M <= 16 activation rows ride as one MFMA operand, a workgroup owns 16 weight rows (a contiguous 16*K*2-byte block of
// HBM), its 8 waves split K, each wave keeps a ring of DEPTH 1 KiB weight loads in flight (non-temporal: the stream must not evict
// the activations from L2) and the 8 partial 16x16 tiles meet in LDS.
//
// Weight forms.  The weight rows are streamed as bf16, as e4m3 codes (fp8: avllm_mx_quantize layout 2) or as OCP MXFP4 codes (fp4: e2m1, two
// per byte, element 2i in the LOW nibble; avllm_mx4_quantize); both code forms carry one E8M0 exponent per 32 elements along K (E8 [*, K/32]
// row-major, biased by 127) and become the same bf16 MFMA operand through v_cvt_scalef32_pk_bf16_fp8 / _fp4 (exact: code x 2^e is a bf16
// value).  A wave's K range, the 8-way split and the 128-column ring group are the same for every form; what a form decides -- 16-byte weight
// loads per group, which K elements lane (fr, fq) multiplies at step j (the activation and norm-weight addresses follow), which exponent byte
// scales them, the order in which a group's loads are issued (the wait counts derive from it), the conversion and the ring depth -- is its
// DecForm below and nowhere else.  So the result is the bf16 form's on the dequantised weights up to fp32 summation order inside a group.
#include "common.h"
#include "avllm_internal.h"
#include "mx.h"
#include <type_traits>

namespace {

constexpr int DW = 8;            // waves per workgroup (K split)

enum { DEC_PLAIN = 0, DEC_SWIGLU = 1, DEC_QKV = 2 };
enum class WForm { bf16 = 0, fp8 = 1, fp4 = 2 };

struct DecArgs {
    const bf16* A; long lda;            // activations [M, K]
    const uint8_t* W; long ldw;         // weight rows [*, K] in the form's elements, ldw BYTES apart
    const uint8_t* E8; WForm form;      // fp8 / fp4: exponents [*, K/32]
    const bf16* norm_w; float eps;      // NORM: A is RMS-normalised on the fly (x * rstd * w)
    int M, K, N, mode;
    void* C; long ldc; int out_f32;     // PLAIN: C[M,N] (+R); SWIGLU: C[M,N=F] = silu(gate) * up; QKV: q part [M, dq]
    const bf16* R; long ldr;
    int F;                              // SWIGLU: weight row of "up" column n is F + n
    int dq, dkv, hd;                    // QKV: columns [0,dq) q, [dq,dq+dkv) k, [dq+dkv, dq+2dkv) v; rotary pairs (i, i + hd/2) inside each head
    const float* rope;                  // [hd/2][2] cos,sin of this position
    bf16* kc; bf16* vc;                 // cache of this layer [M(=B), Tmax, dkv]
    int Tmax, pos; const int* pos_dev;  // row written = pos (+ *pos_dev)
    // LoRA side term (peft lora.Linear: + scale * B (A x)): lt [M, ldlt] f32 holds the rank-side products A x of this projection's input
    // (columns 64 j .. 64 j + r of module j; made by a PLAIN launch over the A images), lb[j] the padded B image [rows, 64] of module j
    // (QKV: j = q, k, v; otherwise j = 0).  Added in the epilogue, before RoPE.
    const float* lt; long ldlt; const bf16* lb[3]; float lscale; int lr;
    // frozen projection bias (Qwen2 q|k|v, attention_bias o): [N] in logical output column order, added to the fp32 sum after the RMS scale,
    // before the adapter term, the residual and RoPE (peft: base_layer(x) with its bias, + adapter).  PLAIN and QKV only.
    const bf16* bias;
    // QKV: columns below rot_end are rotated (their rows paired inside a workgroup), columns below q_end go to C, the rest to the cache.  The
    // fused form has rot_end = dq + dkv, q_end = dq; raw_qkv (a head norm follows: qk_norm.hip) has rot_end = 0, q_end = N: the plain row
    // mapping, no rotation, no cache write.  Run-time data, so both forms are the same kernels.
    int rot_end, q_end;
};

// fragment row fr (0..15) of workgroup b -> weight row, and the logical output column it produces
__device__ __forceinline__ int dec_wrow(const DecArgs& a, int b, int fr, int& col) {
    if (a.mode == DEC_SWIGLU) {
        col = 8 * b + (fr & 7);
        return fr < 8 ? col : a.F + col;
    }
    if (a.mode == DEC_QKV) {
        const int c0 = 16 * b;
        if (c0 < a.rot_end) {           // rotary region: 8 columns of the first half of a head + their 8 partners
            const int per_head = a.hd >> 4;
            const int h = b / per_head, s = b - h * per_head;
            col = h * a.hd + 8 * s + (fr & 7) + (fr < 8 ? 0 : a.hd >> 1);
            return col;
        }
    }
    col = 16 * b + fr;
    return col;
}

// 16-byte global loads the compiler's wait-count pass does not see: the ring below keeps its groups in flight and waits with exact vmcnt
// values (loads return in issue order), which clang does not do for a register ring (it drains to vmcnt(0) every trip).
typedef u32x4 frag;
template <int OFF> __device__ __forceinline__ void gld(frag& r, const void* p) {
    asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(r) : "v"(p), "n"(OFF) : "memory");
}
template <int OFF> __device__ __forceinline__ void gld_nt(frag& r, const void* p) {
    asm volatile("global_load_dwordx4 %0, %1, off offset:%2 nt" : "=v"(r) : "v"(p), "n"(OFF) : "memory");
}
template <int OFF> __device__ __forceinline__ void gld_dw(unsigned& r, const void* p) {
    asm volatile("global_load_dword %0, %1, off offset:%2" : "=v"(r) : "v"(p), "n"(OFF) : "memory");
}
// the wait names the registers the step reads, so nothing that uses them moves above it
template <int N> __device__ __forceinline__ void wait_vm(frag& a, frag& b) {
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}
template <int N> __device__ __forceinline__ void wait_vm(frag& a, frag& b, frag& c) {
    asm volatile("s_waitcnt vmcnt(%3)" : "+v"(a), "+v"(b), "+v"(c) : "n"(N));
}
template <int N> __device__ __forceinline__ void wait_vm(frag& a, frag& b, unsigned& e) {
    asm volatile("s_waitcnt vmcnt(%3)" : "+v"(a), "+v"(b), "+v"(e) : "n"(N));
}
template <int N> __device__ __forceinline__ void wait_vm(frag& a, frag& b, frag& c, unsigned& e) {
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(e) : "n"(N));
}
template <int I, int N, class F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<I + 1, N>(f); }
}

// DPP moves inside each row of 16 lanes (the fr index of an MFMA operand): rotate so that lane i reads lane i + S, or broadcast lane J
template <int CTRL> __device__ __forceinline__ frag dpp4(frag v) {
    frag r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (unsigned)__builtin_amdgcn_update_dpp((int)v[e], (int)v[e], CTRL, 0xf, 0xf, false);
    return r;
}
template <int S> __device__ __forceinline__ frag row_from_higher(frag v) { return dpp4<0x120 + ((16 - S) & 15)>(v); }      // row_ror:(16 - S)
template <int J> __device__ __forceinline__ frag row_bcast(frag v) { return dpp4<0x150 + J>(v); }                           // row_newbcast:J

// One ring group = 4 K-steps of 32.  The weight stream is NOT what limits a projection: a pure read of the same bytes in the same pattern
// runs at 5.6 TB/s, adding one activation load per weight load drops it to 4.0 (tools/ubench/stream_features.hip): the CU's vector-memory
// path is the limiter, so every load that is not a weight load has to go.  AL = activation loads per group:
//   M > 8: 4 (lane (fr, fq) = row fr of one step);  M <= 8: 2 (lanes fr >= 8 fetch rows 0..7 of the NEXT step and a row rotate brings them
//   down when that step is consumed; MFMA output columns >= 8 are garbage nobody reads);  M <= 4: 1 (four steps per load).
// The norm weights of the 4 steps come in ONE load (lane row fr & 3 holds step fr & 3) and reach all rows through a row broadcast; the
// exponents of a weight row's 4 blocks are one dword.

// The loads of one group in issue order.  The wait count of a step is read off this list, so it cannot drift from what issue() does.
enum { LD_W, LD_X, LD_N, LD_E };            // weight load i (16 bytes at byte 64 i of the lane's group), activation load i, norm weights, exponents
struct DecOrder {
    int n = 0, kind[10] = {}, idx[10] = {};
    constexpr void add(int k, int i) { kind[n] = k; idx[n] = i; ++n; }
    constexpr int upto(int k, int i) const {            // loads issued up to and including load (k, i); 0 if the group has none
        for (int p = 0; p < n; ++p) if (kind[p] == k && idx[p] == i) return p + 1;
        return 0;
    }
    // loads the step that reads weight load w and activation load x has to see back (they return in issue order)
    constexpr int through(int w, int x) const {
        int t = upto(LD_W, w);
        for (int u : {upto(LD_X, x), upto(LD_N, 0), upto(LD_E, 0)}) t = u > t ? u : t;
        return t;
    }
};

// A weight form's data format, the only place that knows it.  WL: 16-byte weight loads per lane and 128-column group (step j reads load
// j WL / 4); EXP: the group has an exponent dword; depth: groups in flight, the smaller the group's bytes the deeper; koff: element offset
// inside the group of step j for lane column fq; ebit: bit offset in the exponent dword of the byte that scales those elements; order: see
// DecOrder (SPL = steps per activation load; the orders were measured: profiles/r01_decode_bench.txt, r06_decode_fp8_bench.txt,
// r08_decode_fp4_bench.txt, the last also for depths 2 and 6 of fp4); operand: the step's 8 weights as the bf16 MFMA operand, times sc.
template <WForm F> struct DecForm;
template <> struct DecForm<WForm::bf16> {
    static constexpr int WL = 4;
    static constexpr bool EXP = false;
    static constexpr int depth(int) { return 2; }
    static constexpr int koff(int j, int fq) { return 32 * j + 8 * fq; }
    static constexpr int ebit(int, int) { return 0; }
    static constexpr DecOrder order(int SPL, bool NORM) {           // [norm], then per step: [activation if the step starts a load] weight
        DecOrder o;
        if (NORM) o.add(LD_N, 0);
        for (int j = 0; j < 4; ++j) { if (j % SPL == 0) o.add(LD_X, j / SPL); o.add(LD_W, j); }
        return o;
    }
    template <int J> static __device__ __forceinline__ bf16x8 operand(const frag (&wb)[WL], float) { return __builtin_bit_cast(bf16x8, wb[J]); }
};
template <> struct DecForm<WForm::fp8> {                            // one code load covers TWO steps of a lane: dwords 2 (j & 1), + 1 are step j's
    static constexpr int WL = 2;
    static constexpr bool EXP = true;
    static constexpr int depth(int) { return 2; }
    static constexpr int koff(int j, int fq) { return 64 * (j >> 1) + 16 * fq + 8 * (j & 1); }
    static constexpr int ebit(int j, int fq) { return 16 * (j >> 1) + 8 * (fq >> 1); }
    static constexpr DecOrder order(int SPL, bool NORM) {           // [norm] exponents, then per step: [activation] [codes if the step starts a pair]
        DecOrder o;
        if (NORM) o.add(LD_N, 0);
        o.add(LD_E, 0);
        for (int j = 0; j < 4; ++j) { if (j % SPL == 0) o.add(LD_X, j / SPL); if (j % 2 == 0) o.add(LD_W, j / 2); }
        return o;
    }
    template <int J> static __device__ __forceinline__ bf16x8 operand(const frag (&wb)[WL], float sc) {
        const unsigned c0 = wb[J / 2][2 * (J & 1)], c1 = wb[J / 2][2 * (J & 1) + 1];
        const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c0, sc, false), p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c0, sc, true);
        const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c1, sc, false), p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c1, sc, true);
        return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
    }
};
template <> struct DecForm<WForm::fp4> {                            // one code load covers all FOUR steps: the lane's 32 elements are one MX block, dword j is step j's
    static constexpr int WL = 1;
    static constexpr bool EXP = true;
    static constexpr int depth(int AL) { return AL == 4 ? 3 : 4; }  // AL = 4: 25 ring registers per group
    static constexpr int koff(int j, int fq) { return 32 * fq + 8 * j; }
    static constexpr int ebit(int, int fq) { return 8 * fq; }
    static constexpr DecOrder order(int SPL, bool NORM) {           // codes, [norm], exponents, activations
        DecOrder o;
        o.add(LD_W, 0);
        if (NORM) o.add(LD_N, 0);
        o.add(LD_E, 0);
        for (int i = 0; i < 4 / SPL; ++i) o.add(LD_X, i);
        return o;
    }
    template <int J> static __device__ __forceinline__ bf16x8 operand(const frag (&wb)[WL], float sc) {
        const unsigned c = wb[0][J];
        const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 0), p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 1);
        const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 2), p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 3);
        return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
    }
};

template <WForm F, int AL> struct DecGrp { frag wb[DecForm<F>::WL], xa[AL], gw; unsigned ex; };
template <WForm F, int AL, bool NORM> constexpr DecOrder dec_order = DecForm<F>::order(4 / AL, NORM);

// The K loop of one wave: G groups from column k0 on, accumulated in increasing order.  Ring of D groups with fixed slot roles (a loop whose
// exit alternates between the slots makes the compiler copy ring registers that still have loads in flight): the main loop consumes and
// refills D groups per trip (single exit), the remaining 1 .. 2D-1 groups are a straight-line tail chosen by their count, so every wait
// count is an immediate.  A group is refilled in one burst once its 4 steps are consumed.  A wave with G = 0 (K < 1024: fewer groups than waves) issues and consumes nothing.
template <WForm F, bool NORM, int AL>
__device__ __forceinline__ void dec_k_loop(const DecArgs& a, int fr, int fq, int ar, int asub, int wr, long k0, int G, f32x4& acc, float& ss) {
    typedef DecForm<F> Fm;
    typedef DecGrp<F, AL> Grp;
    constexpr int SPL = 4 / AL, RPL = 16 / SPL, D = Fm::depth(AL), WL = Fm::WL;        // K-steps, activation rows per activation load
    constexpr DecOrder ORD = dec_order<F, AL, NORM>;
    const bf16* ap = a.A + (long)ar * a.lda + k0 + Fm::koff(asub, fq);
    const uint8_t* bp = a.W + (long)wr * a.ldw + (k0 >> 1) * WL + fq * 16;
    const uint8_t* ep = Fm::EXP ? a.E8 + (long)wr * (a.K >> 5) + (k0 >> 5) : nullptr;
    const bf16* gp = NORM ? a.norm_w + k0 + Fm::koff(fr & 3, fq) : a.A;
    Grp s[D];
    auto issue = [&](Grp& g, int grp) {
        static_for<0, ORD.n>([&](auto pc) {
            constexpr int kind = dec_order<F, AL, NORM>.kind[decltype(pc)::value], i = dec_order<F, AL, NORM>.idx[decltype(pc)::value];
            if constexpr (kind == LD_W) gld_nt<64 * i>(g.wb[i], bp + (long)grp * (64 * WL));
            else if constexpr (kind == LD_X) gld<2 * Fm::koff(SPL * i, 0)>(g.xa[i], ap + (long)grp * 128);
            else if constexpr (kind == LD_N) gld<0>(g.gw, gp + (long)grp * 128);
            else gld_dw<0>(g.ex, ep + (long)grp * 4);
        });
    };
    auto step = [&](Grp& g, auto jc, auto behind) {      // wait for step j of this group (`behind` younger groups in flight), multiply
        constexpr int j = decltype(jc)::value, wl = j * WL / 4, xl = j / SPL;
        constexpr int N = dec_order<F, AL, NORM>.n * (1 + decltype(behind)::value) - dec_order<F, AL, NORM>.through(wl, xl);
        if constexpr (NORM && Fm::EXP) wait_vm<N>(g.wb[wl], g.xa[xl], g.gw, g.ex);
        else if constexpr (NORM) wait_vm<N>(g.wb[wl], g.xa[xl], g.gw);
        else if constexpr (Fm::EXP) wait_vm<N>(g.wb[wl], g.xa[xl], g.ex);
        else wait_vm<N>(g.wb[wl], g.xa[xl]);
        frag xr = g.xa[xl];
        if constexpr (j % SPL != 0) xr = row_from_higher<RPL * (j % SPL)>(xr);
        bf16x8 x = __builtin_bit_cast(bf16x8, xr);
        if constexpr (NORM) {
            const bf16x8 gv = __builtin_bit_cast(bf16x8, row_bcast<j>(g.gw));
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xf = (float)x[e];
                ss += xf * xf;
                x[e] = (bf16)(xf * (float)gv[e]);
            }
        }
        float sc = 0.f;                                  // 2^(e - 127) of the lane's block
        if constexpr (Fm::EXP) sc = mx_e8m0((g.ex >> Fm::ebit(j, fq)) & 0xffu);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Fm::template operand<j>(g.wb, sc), x, acc, 0, 0, 0);      // D[n][m]
    };
    auto consume = [&](Grp& g, auto behind) { static_for<0, 4>([&](auto jc) { step(g, jc, behind); }); };
    static_for<0, D>([&](auto ic) { if (decltype(ic)::value < G) issue(s[decltype(ic)::value], decltype(ic)::value); });
    int g = 0;
    for (; g + 2 * D <= G; g += D)
        static_for<0, D>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            consume(s[i], std::integral_constant<int, D - 1>{});
            issue(s[i], g + D + i);
        });
    const int rem = G - g;
    static_for<1, 2 * D>([&](auto tc) {
        constexpr int T = decltype(tc)::value;
        if (rem == T)
            static_for<0, T>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                consume(s[i % D], std::integral_constant<int, (T < i + D ? T : i + D) - 1 - i>{});     // younger groups in flight
                if constexpr (i + D < T) issue(s[i % D], g + D + i);
            });
    });
}

template <WForm F, bool NORM, int AL, bool LORA, bool BIAS = false>
__device__ __forceinline__ void dec_proj_body(const DecArgs& a) {
    __shared__ float part[DW][16][17];      // [wave][n][m]
    __shared__ float ssq[DW][16];
    __shared__ float fin[16][17];           // [m][n]
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int M = a.M;
    constexpr int RPL = 4 * AL;              // activation rows per load (16 / K-steps per load)
    const int arow = fr & (RPL - 1), asub = fr / RPL;
    const int ar = arow < M ? arow : M - 1;
    // K in units of 4 steps (128 columns), dealt to the 8 waves as evenly as whole units allow (K = 11008: 11,11,11,11,11,11,10,10)
    const int U = a.K >> 7, ub = U / DW, ue = U - ub * DW;
    const int G = ub + (w < ue ? 1 : 0);
    const long k0 = ((long)w * ub + (w < ue ? w : ue)) << 7;
    int col;
    const int wr = dec_wrow(a, blockIdx.x, fr, col);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float ss = 0.f;
    dec_k_loop<F, NORM, AL>(a, fr, fq, ar, asub, wr, k0, G, acc, ss);
    // adapters: the finishing thread (m, nn) fetches its 16 rank-side products and its B row now (the weight ring has drained; the loads
    // fly while the partial tiles meet in LDS)
    f32x4 ltv[4] = {};
    bf16x8 lbv[2] = {};
    if constexpr (LORA) {
        if (threadIdx.x < 256 && (int)(threadIdx.x >> 4) < M) {
            int oc;
            dec_wrow(a, blockIdx.x, threadIdx.x & 15, oc);
            int j = 0, row = oc;
            if (a.mode == DEC_QKV) { j = oc < a.dq ? 0 : (oc < a.dq + a.dkv ? 1 : 2); row = oc - (j == 0 ? 0 : (j == 1 ? a.dq : a.dq + a.dkv)); }
            if (oc < a.N) {
                const float* tp = a.lt + (long)(threadIdx.x >> 4) * a.ldlt + 64 * j;
                const bf16* bp2 = a.lb[j] + (long)row * 64;
#pragma unroll
                for (int i = 0; i < 4; ++i) ltv[i] = *(const f32x4*)(tp + 4 * i);
                lbv[0] = *(const bf16x8*)bp2;
                lbv[1] = *(const bf16x8*)(bp2 + 8);
            }
        }
    }
    // bias of the finishing thread's column, fetched with the adapter operands.  BIAS is a template parameter, not a run-time test: a
    // wave-uniform `if (a.bias)` in the one kernel measured slower or equal in all nine cells of the bias-free Llama-2-7B token step (mean
    // +5 us, 0.15 %; three cells beyond the round-to-round spread: profiles/r09_decode_bias_bench.txt), so a launch without a bias (every
    // Llama checkpoint) runs the kernels it always ran
    float bv = 0.f;
    if constexpr (BIAS) {
        if (threadIdx.x < 256) {
            int oc;
            dec_wrow(a, blockIdx.x, threadIdx.x & 15, oc);
            if (oc < a.N) bv = (float)a.bias[oc];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) part[w][fq * 4 + i][fr] = acc[i];
    if (NORM) {
        ss += __shfl_xor(ss, 16);
        ss += __shfl_xor(ss, 32);
        if (fq == 0) ssq[w][fr] = ss;
    }
    __syncthreads();
    if (threadIdx.x >= 256) return;
    const int m = threadIdx.x >> 4, nn = threadIdx.x & 15;
    float s = 0.f;
#pragma unroll
    for (int x = 0; x < DW; ++x) s += part[x][nn][m];
    if (NORM) {
        float t = 0.f;
#pragma unroll
        for (int x = 0; x < DW; ++x) t += ssq[x][m];
        s *= rsqrtf(t / (float)a.K + a.eps);
    }
    if constexpr (BIAS) s += bv;
    if constexpr (LORA) {
        float u = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) u += (i < a.lr ? ltv[i >> 2][i & 3] : 0.f) * (float)lbv[i >> 3][i & 7];
        s += a.lscale * u;
    }
    int ocol;
    dec_wrow(a, blockIdx.x, nn, ocol);
    if (a.mode == DEC_PLAIN) {
        if (m < M && ocol < a.N) {
            if (a.R) s += (float)a.R[(long)m * a.ldr + ocol];
            if (a.out_f32) ((float*)a.C)[(long)m * a.ldc + ocol] = s;
            else ((bf16*)a.C)[(long)m * a.ldc + ocol] = (bf16)s;
        }
        return;
    }
    fin[m][nn] = s;
    __syncthreads();                         // all 256 remaining threads reach it (4 whole waves)
    if (m >= M) return;
    const float other = fin[m][nn ^ 8];
    if (a.mode == DEC_SWIGLU) {
        if (nn < 8) ((bf16*)a.C)[(long)m * a.ldc + ocol] = (bf16)(s / (1.0f + __expf(-s)) * other);
        return;
    }
    // DEC_QKV
    const int pos = a.pos + (a.pos_dev ? *a.pos_dev : 0);
    float o = s;
    if (ocol < a.rot_end) {
        const int i = (ocol % a.hd) & ((a.hd >> 1) - 1);
        const float c = a.rope[2 * i], sn = a.rope[2 * i + 1];
        o = nn < 8 ? s * c - other * sn : s * c + other * sn;
    }
    // position from device memory: the host could not check it.  A step replayed past the end of the cache writes nothing (the cache
    // rows of the last valid position stay as they are) instead of running over [B, Tmax, dkv]; attn_decode1_kernel clamps its length alike.
    const bool in_cache = pos >= 0 && pos < a.Tmax;
    if (ocol < a.q_end) ((bf16*)a.C)[(long)m * a.ldc + ocol] = (bf16)o;
    else if (!in_cache) return;
    else if (ocol < a.dq + a.dkv) a.kc[((long)m * a.Tmax + pos) * a.dkv + ocol - a.dq] = (bf16)o;
    else a.vc[((long)m * a.Tmax + pos) * a.dkv + ocol - a.dq - a.dkv] = (bf16)o;
}

template <bool NORM, int AL, bool LORA>
__global__ __launch_bounds__(DW * 64, 2) void dec_proj_kernel(DecArgs a) { dec_proj_body<WForm::bf16, NORM, AL, LORA>(a); }
template <bool NORM, int AL, bool LORA>
__global__ __launch_bounds__(DW * 64, 2) void dec_proj_f8_kernel(DecArgs a) { dec_proj_body<WForm::fp8, NORM, AL, LORA>(a); }
template <bool NORM, int AL, bool LORA>
__global__ __launch_bounds__(DW * 64, 2) void dec_proj_f4_kernel(DecArgs a) { dec_proj_body<WForm::fp4, NORM, AL, LORA>(a); }

// the same with a bias (modes 0 and 2 only)
template <bool NORM, int AL, bool LORA>
__global__ __launch_bounds__(DW * 64, 2) void dec_bias_kernel(DecArgs a) { dec_proj_body<WForm::bf16, NORM, AL, LORA, true>(a); }
template <bool NORM, int AL, bool LORA>
__global__ __launch_bounds__(DW * 64, 2) void dec_bias_f8_kernel(DecArgs a) { dec_proj_body<WForm::fp8, NORM, AL, LORA, true>(a); }
template <bool NORM, int AL, bool LORA>
__global__ __launch_bounds__(DW * 64, 2) void dec_bias_f4_kernel(DecArgs a) { dec_proj_body<WForm::fp4, NORM, AL, LORA, true>(a); }

}  // namespace

bool av_dec_proj_supported(int dtype, int M, int K, int N, int mode, int hd) {
    if (dtype != AV_BF16 || M < 1 || M > 16 || K % 128 != 0) return false;
    if (mode == DEC_SWIGLU) return N % 8 == 0;
    // the rotary index of a column is (col % hd) & (hd / 2 - 1): a mask, so hd has to be a power of two (32, 64, 128, ...)
    if (mode == DEC_QKV) return N % 16 == 0 && hd >= 32 && (hd & (hd - 1)) == 0;
    return N % 16 == 0;
}

static int dec_launch(DecArgs& a, hipStream_t st) {
    // [form][norm][al: 1, 2, 4][adapters]
#define DEC_FORM_TABLE(K) {{{K<false, 1, false>, K<false, 1, true>}, {K<false, 2, false>, K<false, 2, true>}, {K<false, 4, false>, K<false, 4, true>}}, \
                           {{K<true, 1, false>, K<true, 1, true>}, {K<true, 2, false>, K<true, 2, true>}, {K<true, 4, false>, K<true, 4, true>}}}
    static const decltype(&dec_proj_kernel<false, 1, false>) kernel[3][2][3][2] = {DEC_FORM_TABLE(dec_proj_kernel), DEC_FORM_TABLE(dec_proj_f8_kernel),
                                                                                   DEC_FORM_TABLE(dec_proj_f4_kernel)};
    static const decltype(&dec_proj_kernel<false, 1, false>) kernel_bias[3][2][3][2] = {DEC_FORM_TABLE(dec_bias_kernel), DEC_FORM_TABLE(dec_bias_f8_kernel),
                                                                                        DEC_FORM_TABLE(dec_bias_f4_kernel)};
#undef DEC_FORM_TABLE
    const int grid = a.mode == DEC_SWIGLU ? a.N / 8 : a.N / 16;
    const int ev = av_knob(AV_KNOB_DEC_AL);       // experiment knob: force the activation-load form (4 = one load per step)
    const int al = ev ? ev : (a.M <= 4 ? 1 : a.M <= 8 ? 2 : 4);
    const int ali = al == 1 && a.M <= 4 ? 0 : al <= 2 && a.M <= 8 ? 1 : 2;
    hipLaunchKernelGGL((a.bias ? kernel_bias : kernel)[(int)a.form][a.norm_w != nullptr][ali][a.lt != nullptr], dim3(grid), dim3(DW * 64), 0, st, a);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_dec_proj(const avllm_dec_proj_desc* d, hipStream_t st) {
    AV_CHECK_ARG(d && d->A && (d->W || d->W8 || d->W4), "dec_proj: null operand");
    AV_CHECK_ARG(!(d->W8 && d->W4), "dec_proj: W8 and W4 are two forms of the same weights, give one");
    AV_CHECK_ARG(d->mode >= DEC_PLAIN && d->mode <= DEC_QKV, "dec_proj: mode %d", d->mode);
    AV_CHECK_ARG(av_dec_proj_supported(AV_BF16, d->M, d->K, d->N, d->mode, d->hd),
                 "dec_proj: bf16, 1 <= M <= 16 (M=%d), K %% 128 == 0 (K=%d), N %% 16 == 0 (%% 8 for SwiGLU; N=%d), q|k|v: head dim a power of two >= 32 (hd=%d)",
                 d->M, d->K, d->N, d->hd);
    AV_CHECK_ARG(d->lda % 8 == 0 && d->ldw % 8 == 0 && d->lda >= d->K && d->ldw >= (d->W4 ? d->K / 2 : d->K),
                 "dec_proj: rows must be 16-byte aligned and hold K elements");
    // the public descriptor names the form by the pointer that is set (ldw: bf16 elements, or bytes of codes); the kernels take one pointer
    const WForm form = d->W4 ? WForm::fp4 : d->W8 ? WForm::fp8 : WForm::bf16;
    const void* W = d->W4 ? d->W4 : d->W8 ? d->W8 : d->W;
    AV_CHECK_ARG(form == WForm::bf16 || (d->E8 && ((uintptr_t)W & 15) == 0 && d->ldw % 16 == 0 && ((uintptr_t)d->E8 & 3) == 0),
                 "dec_proj(%s weights): codes 16-byte aligned with rows of ldw %% 16 == 0 bytes (ldw=%ld), exponents E8 [rows, K/32] 4-byte aligned",
                 form == WForm::fp4 ? "fp4" : "fp8", (long)d->ldw);
    DecArgs a = {};
    a.W = (const uint8_t*)W; a.ldw = form == WForm::bf16 ? 2 * d->ldw : d->ldw; a.E8 = (const uint8_t*)d->E8; a.form = form;
    a.A = (const bf16*)d->A; a.lda = d->lda; a.norm_w = (const bf16*)d->norm_w; a.eps = d->eps;
    a.M = d->M; a.K = d->K; a.N = d->N; a.mode = d->mode;
    a.C = d->C; a.ldc = d->ldc; a.out_f32 = d->out_f32; a.R = (const bf16*)d->R; a.ldr = d->ldr;
    if (d->mode == DEC_PLAIN) {
        AV_CHECK_ARG(d->C && d->ldc >= d->N && (!d->R || d->ldr >= d->N), "dec_proj: output [M,N] missing or rows shorter than N");
    } else if (d->mode == DEC_SWIGLU) {
        AV_CHECK_ARG(d->C && d->ldc >= d->N && !d->R && !d->out_f32, "dec_proj(SwiGLU): bf16 output [M,F] without residual");
        a.F = d->N;
    } else {
        const bool raw = d->raw_qkv != 0;
        AV_CHECK_ARG(d->C && (raw || (d->kc && d->vc && d->rope)) && d->dq > 0 && d->dkv > 0 && d->N == d->dq + 2 * d->dkv && d->dq % d->hd == 0 &&
                     d->dkv % d->hd == 0 && d->ldc >= (raw ? d->N : d->dq) && !d->R && !d->out_f32,
                     "dec_proj(q|k|v): N=%d must be dq + 2 dkv (dq=%d dkv=%d) in whole heads of %d; raw_qkv: ldc >= N", d->N, d->dq, d->dkv, d->hd);
        a.dq = d->dq; a.dkv = d->dkv; a.hd = d->hd;
        if (raw) { a.rot_end = 0; a.q_end = d->N; }
        else {
            AV_CHECK_ARG(d->Tmax > 0 && d->pos >= 0 && (d->pos_dev || d->pos < d->Tmax), "dec_proj(q|k|v): pos=%d outside the cache (Tmax=%d)", d->pos, d->Tmax);
            a.rot_end = d->dq + d->dkv; a.q_end = d->dq;
            a.rope = d->rope; a.kc = (bf16*)d->kc; a.vc = (bf16*)d->vc; a.Tmax = d->Tmax; a.pos = d->pos; a.pos_dev = d->pos_dev;
        }
    }
    if (d->lora_t) {
        const int nmod = d->mode == DEC_QKV ? 3 : 1;
        AV_CHECK_ARG(d->mode != DEC_SWIGLU && d->lora_r > 0 && d->lora_r <= 16 && d->ld_lora_t >= 64 * nmod && d->ld_lora_t % 4 == 0 &&
                     ((uintptr_t)d->lora_t & 15) == 0, "dec_proj: adapters need rank <= 16 (r=%d), 16-byte aligned rank-side products with >= %d columns per row",
                     d->lora_r, 64 * nmod);
        for (int j = 0; j < nmod; ++j) AV_CHECK_ARG(d->lora_b[j], "dec_proj: adapter B image %d missing", j);
        a.lt = d->lora_t; a.ldlt = d->ld_lora_t; a.lscale = d->lora_scale; a.lr = d->lora_r;
        for (int j = 0; j < nmod; ++j) a.lb[j] = (const bf16*)d->lora_b[j];
    }
    if (d->bias) {
        AV_CHECK_ARG(d->mode != DEC_SWIGLU && ((uintptr_t)d->bias & 1) == 0, "dec_proj: a bias [N] (bf16, 2-byte aligned) goes with modes 0 and 2, not SwiGLU (mode=%d)",
                     d->mode);
        a.bias = (const bf16*)d->bias;
    }
    return dec_launch(a, st);
}

extern "C" int avllm_dec_proj(const avllm_dec_proj_desc* d, void* stream) { return av_dec_proj(d, (hipStream_t)stream); }

__global__ void pos_advance_kernel(int* p, int by) { if (threadIdx.x == 0 && blockIdx.x == 0) *p += by; }

extern "C" int avllm_pos_advance(int32_t* pos_dev, int32_t by, void* stream) {
    AV_CHECK_ARG(pos_dev, "pos_advance: null");
    hipLaunchKernelGGL(pos_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, pos_dev, by);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
