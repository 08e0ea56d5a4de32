// The row forms of the single-token attention kernels (attention_decode.hip, attention_decode_shared.hip): what a KV cache form decides and
// nothing else.  Include INSIDE the anonymous namespace of the file that instantiates them (after common.h and mx.h), so the kernels' mangled
// names and code stay those of a form defined in the file itself.
//   PlainRow<T>  bf16 or float rows [B, Tmax, Hkv hd]: a lane owns N = 8 elements of a row
//   E4m3Row      the block-scaled image of kv_fp8.hip: a lane owns N = 16 codes of a row (one 16-byte load + the block's exponent byte).
//                Dequantisation is exact: code x 2^e, the power of two applied once to the lane's partial score and once to the softmax weight.
// A row form supplies N, the q / output element type Elem, the cache arguments Cache, what a lane holds in flight of one K or one V row (Raw),
// zero(k, v), load(t, k, v), dot(qv, k) (the lane's partial score) and values(v, vf) (the lane's V elements in fp32; returns the factor the
// softmax weight takes).

template <typename T> struct PlainRow {
    static constexpr int N = 8;
    typedef T Elem;
    struct Cache { const T *k, *v; };                            // [B, Tmax, d]
    struct Raw { float x[8]; };
    const T *kbase, *vbase; int d;
    // lane columns [dc N, dc N + N) of kv head hk of sequence b; d = row width
    __device__ __forceinline__ PlainRow(const Cache& c, int b, int Tmax, int d_, int hk, int hd, int dc)
        : kbase(c.k + ((long)b * Tmax) * d_ + (long)hk * hd + dc * 8), vbase(c.v + ((long)b * Tmax) * d_ + (long)hk * hd + dc * 8), d(d_) {}
    static __device__ __forceinline__ void zero(Raw& k, Raw& v) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { k.x[j] = 0.f; v.x[j] = 0.f; }
    }
    __device__ __forceinline__ void load(int t, Raw& k, Raw& v) const { load_f<8>(kbase + (long)t * d, k.x); load_f<8>(vbase + (long)t * d, v.x); }
    static __device__ __forceinline__ float dot(const float (&qv)[8], const Raw& k) {
        float x = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) x += qv[j] * k.x[j];
        return x;
    }
    static __device__ __forceinline__ float values(const Raw& v, float (&vf)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) vf[j] = v.x[j];
        return 1.f;
    }
};

struct E4m3Row {
    static constexpr int N = 16;
    typedef bf16 Elem;
    struct Cache { const uint8_t *kq, *ke, *vq, *ve; };          // codes [B, Tmax, d], exponents [B, Tmax, d/32] of K and of V
    struct Raw { u32x4 c; unsigned x; };
    Cache c; long cbase, ebase; int d, de;
    __device__ __forceinline__ E4m3Row(const Cache& c_, int b, int Tmax, int d_, int hk, int hd, int dc)
        : c(c_), cbase(((long)b * Tmax) * d_ + (long)hk * hd + dc * 16), ebase(((long)b * Tmax) * (d_ >> 5) + hk * (hd >> 5) + (dc >> 1)), d(d_),
          de(d_ >> 5) {}
    static __device__ __forceinline__ void zero(Raw& k, Raw& v) { k.c = (u32x4){0u, 0u, 0u, 0u}; v.c = (u32x4){0u, 0u, 0u, 0u}; k.x = 0u; v.x = 0u; }
    __device__ __forceinline__ void load(int t, Raw& k, Raw& v) const {
        k.c = *(const u32x4*)(c.kq + cbase + (long)t * d);
        v.c = *(const u32x4*)(c.vq + cbase + (long)t * d);
        k.x = c.ke[ebase + (long)t * de];
        v.x = c.ve[ebase + (long)t * de];
    }
    static __device__ __forceinline__ float dot(const float (&qv)[16], const Raw& r) {
        float kf[16], x = 0.f;
        mx_codes16(r.c, kf);
#pragma unroll
        for (int j = 0; j < 16; ++j) x += qv[j] * kf[j];
        return x * mx_e8m0(r.x);
    }
    static __device__ __forceinline__ float values(const Raw& r, float (&vf)[16]) {
        mx_codes16(r.c, vf);
        return mx_e8m0(r.x);
    }
};
