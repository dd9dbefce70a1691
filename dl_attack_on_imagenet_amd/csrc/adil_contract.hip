// ADiL dictionary contractions for gfx950 on the matrix cores.
//   synth :  out = x + vp D^T                 (B x Kp)(Kp x P), fused add / clamps        [K1, K9]
//   grad  :  grad_d = g^T vp (P x K)  and  grad_vb = g D (B x K) in ONE pass over g       [K2, K3, K6]
// D is P x K row-major (atom innermost), image streams are B x P row-major (fp32 or bf16).
//
// Both kernels are HBM-bound streaming kernels; MFMA is used only so that the small dense contractions do not
// become ALU-bound.  One code path per stream type, selected by Mma<T>:
//   T = float  : six v_mfma_f32_32x32x16_bf16 on a three-way bf16 split of each fp32 operand (fp32-grade; the parity path)
//   T = bf16   : v_mfma_f32_32x32x16_bf16 (D and V rounded to bf16 on the fly, fp32 accumulate; the throughput path)
// Every operand fragment covers a "k-group" of 16 reduction indices: lane (r = lane&31, h = lane>>5) supplies the
// 8 consecutive indices 16g + 8h + j, j = 0..7, of row/column r — identical for both instruction shapes, so the
// data movement is shared and only Mma<T>::mma differs (6 split MFMAs vs 1 bf16 MFMA per k-group).
// C/D layout of a 32x32 tile: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <unordered_map>

#include "adil_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // native 16-byte register quad (HIP's uint4 struct resists SROA)
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <typename T> struct Mma;

// fp32 operands on the bf16 matrix pipe.  gfx950 has no xf32 MFMA and v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16
// rate, which made every fp32 contraction MFMA-bound (grad 272 us = 0.17 of the HBM roof in round 1).  Each fp32 value is
// split into three bf16 pieces, x = h + m + l exactly to 2^-24 relative (h = rne(x), m = rne(x - h), l = rne(x - h - m);
// the subtractions are exact), and a product is formed from the six piece products whose weight is >= 2^-16 relative:
//     a b = ah bh + (ah bm + am bh) + (am bm + ah bl + al bh)  + O(2^-24 |a b|)
// — six v_mfma_f32_32x32x16_bf16 per k-group of 16 instead of eight 32x32x2_f32: 192 vs 512 MFMA cycles, fp32
// accumulation, and an error per product of the size of one fp32 rounding (bf16 x bf16 products are exact in fp32).
// Small terms are issued first so that they are not absorbed by a large partial sum.
template <> struct Mma<float> {
    static constexpr bool SCALED = false;
    struct Frag { bf16x8 h, m, l; };
    typedef float Elem;                         // element type of operands staged in LDS / workspace
    static constexpr int PAD = 4;               // LDS row padding (elements): (stride/4) odd -> conflict-free b128
    static __device__ __forceinline__ void mma(f32x16& acc, const Frag& a, const Frag& b) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.l, b.h, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.l, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.m, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.h, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.m, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.h, acc, 0, 0, 0);
    }
    static __device__ __forceinline__ void split2(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
        h = pack2_bf16(x0, x1);
        float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xffff0000u);
        m = pack2_bf16(r0, r1);
        r0 -= __uint_as_float(m << 16);
        r1 -= __uint_as_float(m & 0xffff0000u);
        l = pack2_bf16(r0, r1);
    }
    static __device__ __forceinline__ Frag from8(const float (&f)[8]) {
        u32x4 h, m, l;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned hj, mj, lj;
            split2(f[2 * j], f[2 * j + 1], hj, mj, lj);
            h[j] = hj; m[j] = mj; l[j] = lj;
        }
        Frag r;
        r.h = __builtin_bit_cast(bf16x8, h);
        r.m = __builtin_bit_cast(bf16x8, m);
        r.l = __builtin_bit_cast(bf16x8, l);
        return r;
    }
    static __device__ __forceinline__ void touch(Frag& f) {          // make the value opaque: its loads must have landed
        u32x4 h = __builtin_bit_cast(u32x4, f.h), m = __builtin_bit_cast(u32x4, f.m), l = __builtin_bit_cast(u32x4, f.l);
        asm volatile("" : "+v"(h), "+v"(m), "+v"(l));
        f.h = __builtin_bit_cast(bf16x8, h);
        f.m = __builtin_bit_cast(bf16x8, m);
        f.l = __builtin_bit_cast(bf16x8, l);
    }
    static __device__ __forceinline__ Frag load8(const Elem* p) {      // 8 consecutive elements, 16-B aligned
        const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
        const float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        return from8(f);
    }
    // long-lived fragments are kept un-split (8 registers instead of 12) and expanded where they are used
    struct Raw { float v[8]; };
    static __device__ __forceinline__ Raw load8_raw(const Elem* p) {
        const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
        return Raw{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
    }
    static __device__ __forceinline__ Frag expand(const Raw& r) { return from8(r.v); }
    static __device__ __forceinline__ void touch_raw(Raw& r) {
#pragma unroll
        for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(r.v[j]));
    }
};

template <> struct Mma<bf16_t> {
    static constexpr bool SCALED = false;
    typedef bf16x8 Frag;
    typedef bf16_t Elem;
    static constexpr int PAD = 8;               // (stride*2/16) odd
    static __device__ __forceinline__ void mma(f32x16& acc, const Frag& a, const Frag& b) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
    static __device__ __forceinline__ Frag from8(const float (&f)[8]) {
        u32x4 t;
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = pack2_bf16(f[2 * j], f[2 * j + 1]);
        return __builtin_bit_cast(Frag, t);
    }
    static __device__ __forceinline__ void touch(Frag& f) {
        u32x4 t = __builtin_bit_cast(u32x4, f);
        asm volatile("" : "+v"(t));
        f = __builtin_bit_cast(Frag, t);
    }
    static __device__ __forceinline__ Frag load8(const Elem* p) { return *reinterpret_cast<const Frag*>(p); }
    typedef Frag Raw;
    static __device__ __forceinline__ Raw load8_raw(const Elem* p) { return load8(p); }
    static __device__ __forceinline__ Frag expand(const Raw& r) { return r; }
    static __device__ __forceinline__ void touch_raw(Raw& r) { touch(r); }
};

// fp8 (OCP e4m3 on gfx950) operands for the D.V contraction of the synthesis (BASELINE.json configs[4]): both operands
// are SCALED into the e4m3 range before conversion (codes by vscale = 384 / max|v|, the dictionary by dscale = 256:
// |D| <= 1 is an invariant of update_d, adil.py:33-35) and the fp32 accumulator is scaled back by 1 / (vscale dscale).
// Same fragment geometry as bf16 (lane (r, h) supplies reduction indices 16 g + 8 h + j), 8 bytes per fragment,
// v_mfma_f32_32x32x16_fp8_fp8: twice the bf16 MFMA rate, half the LDS bytes per D-slice read.
struct fp8_t { unsigned char bits; };
struct OpScale { float v, d, o; };              // code scale, dictionary scale, output scale 1 / (v d)
__device__ __forceinline__ float fp8_range(float x) { return fminf(fmaxf(x, -448.0f), 448.0f); }   // e4m3 max normal
template <> struct Mma<fp8_t> {
    typedef long Frag;
    static constexpr bool SCALED = true;
    static __device__ __forceinline__ void mma(f32x16& acc, const Frag& a, const Frag& b) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a, b, acc, 0, 0, 0);
    }
    static __device__ __forceinline__ unsigned pack4(float a, float b, float c, float d) {
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_range(a), fp8_range(b), w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_range(c), fp8_range(d), w, true);
        return (unsigned)w;
    }
    static __device__ __forceinline__ Frag from8(const float (&f)[8]) {       // values already scaled
        const unsigned lo = pack4(f[0], f[1], f[2], f[3]), hi = pack4(f[4], f[5], f[6], f[7]);
        return (long)(((unsigned long)hi << 32) | (unsigned long)lo);
    }
    static __device__ __forceinline__ void touch(Frag& f) { asm volatile("" : "+v"(f)); }
};

// ---- the dictionary operand staged in LDS ------------------------------------------------------------------- //
// Always bf16 elements, row stride n + DPAD.  bf16 streams keep one plane (D rounded to bf16); fp32 streams keep the
// THREE planes h, m, l of Mma<float>'s split, written once per workgroup when the slice / tile is staged: the shared
// operand is then read by every wave as three ds_read_b128 with no conversion work (splitting it at each use made
// the fp32 kernels VALU-bound: 44 VALU per fragment, re-done by every wave for every batch block).
#define DPAD 8
template <typename T> struct DImg;
template <> struct DImg<bf16_t> {
    typedef bf16_t Elem;
    static constexpr int PLANES = 1;
    static __device__ __forceinline__ void put(bf16_t* img, int off, int plane, float v) { (void)plane; img[off] = f32_to_bf16(v); }
    static __device__ __forceinline__ void put2(bf16_t* img, int off, int plane, const float (&f)[2]) {
        (void)plane;
        *reinterpret_cast<unsigned*>(img + off) = pack2_bf16(f[0], f[1]);
    }
    static __device__ __forceinline__ void put4(bf16_t* img, int off, int plane, const float (&f)[4]) {
        (void)plane;
        *reinterpret_cast<u32x2*>(img + off) = u32x2{pack2_bf16(f[0], f[1]), pack2_bf16(f[2], f[3])};
    }
    static __device__ __forceinline__ bf16x8 load8(const bf16_t* p, int plane) {
        (void)plane;
        return *reinterpret_cast<const bf16x8*>(p);
    }
};
template <> struct DImg<float> {
    typedef bf16_t Elem;
    static constexpr int PLANES = 3;
    static __device__ __forceinline__ void put2(bf16_t* img, int off, int plane, const float (&f)[2]) {
        unsigned h, m, l;
        Mma<float>::split2(f[0], f[1], h, m, l);
        *reinterpret_cast<unsigned*>(img + off) = h;
        *reinterpret_cast<unsigned*>(img + off + plane) = m;
        *reinterpret_cast<unsigned*>(img + off + 2 * plane) = l;
    }
    static __device__ __forceinline__ void put4(bf16_t* img, int off, int plane, const float (&f)[4]) {
        unsigned h0, m0, l0, h1, m1, l1;
        Mma<float>::split2(f[0], f[1], h0, m0, l0);
        Mma<float>::split2(f[2], f[3], h1, m1, l1);
        *reinterpret_cast<u32x2*>(img + off) = u32x2{h0, h1};
        *reinterpret_cast<u32x2*>(img + off + plane) = u32x2{m0, m1};
        *reinterpret_cast<u32x2*>(img + off + 2 * plane) = u32x2{l0, l1};
    }
    static __device__ __forceinline__ void put(bf16_t* img, int off, int plane, float v) {
        unsigned h, m, l;
        Mma<float>::split2(v, 0.0f, h, m, l);
        img[off] = (bf16_t)(h & 0xffffu);
        img[off + plane] = (bf16_t)(m & 0xffffu);
        img[off + 2 * plane] = (bf16_t)(l & 0xffffu);
    }
    static __device__ __forceinline__ Mma<float>::Frag load8(const bf16_t* p, int plane) {
        Mma<float>::Frag r;
        r.h = *reinterpret_cast<const bf16x8*>(p);
        r.m = *reinterpret_cast<const bf16x8*>(p + plane);
        r.l = *reinterpret_cast<const bf16x8*>(p + 2 * plane);
        return r;
    }
};

template <> struct DImg<fp8_t> {                 // one byte per element, values pre-scaled by OpScale::d
    typedef unsigned char Elem;                  // row stride Kp + DPAD bytes: an odd number of 8-byte slots (Kp % 16 == 0)
    static constexpr int PLANES = 1;
    static __device__ __forceinline__ void put(unsigned char* img, int off, int plane, float v) {
        (void)plane;
        img[off] = (unsigned char)(Mma<fp8_t>::pack4(v, 0.0f, 0.0f, 0.0f) & 0xffu);
    }
    static __device__ __forceinline__ void put2(unsigned char* img, int off, int plane, const float (&f)[2]) {
        (void)plane;
        *reinterpret_cast<unsigned short*>(img + off) = (unsigned short)(Mma<fp8_t>::pack4(f[0], f[1], 0.0f, 0.0f) & 0xffffu);
    }
    static __device__ __forceinline__ void put4(unsigned char* img, int off, int plane, const float (&f)[4]) {
        (void)plane;
        *reinterpret_cast<unsigned*>(img + off) = Mma<fp8_t>::pack4(f[0], f[1], f[2], f[3]);
    }
    static __device__ __forceinline__ long load8(const unsigned char* p, int plane) {
        (void)plane;
        return *reinterpret_cast<const long*>(p);
    }
};

// ---- image-stream access: N consecutive pixels of one row as floats ---------------------------------------- //
template <typename T, int N> struct PixVec;
template <> struct PixVec<float, 4> {
    static __device__ __forceinline__ void load(const float* p, float (&o)[4]) {
        const float4 t = *reinterpret_cast<const float4*>(p); o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    }
    static __device__ __forceinline__ void store(float* p, const float (&o)[4]) {
        *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
    }
};
template <> struct PixVec<bf16_t, 4> {
    static __device__ __forceinline__ void load(const bf16_t* p, float (&o)[4]) {
        const uint2 t = *reinterpret_cast<const uint2*>(p);
        o[0] = __uint_as_float(t.x << 16); o[1] = __uint_as_float(t.x & 0xffff0000u);
        o[2] = __uint_as_float(t.y << 16); o[3] = __uint_as_float(t.y & 0xffff0000u);
    }
    static __device__ __forceinline__ void store(bf16_t* p, const float (&o)[4]) {
        uint2 t;
        t.x = pack2_bf16(o[0], o[1]);
        t.y = pack2_bf16(o[2], o[3]);
        *reinterpret_cast<uint2*>(p) = t;
    }
};
template <> struct PixVec<float, 2> {
    static __device__ __forceinline__ void load(const float* p, float (&o)[2]) {
        const float2 t = *reinterpret_cast<const float2*>(p); o[0] = t.x; o[1] = t.y;
    }
};
template <> struct PixVec<bf16_t, 2> {
    static __device__ __forceinline__ void load(const bf16_t* p, float (&o)[2]) {
        const unsigned t = *reinterpret_cast<const unsigned*>(p);
        o[0] = __uint_as_float(t << 16); o[1] = __uint_as_float(t & 0xffff0000u);
    }
};
template <typename T> struct PixVec<T, 1> {
    static __device__ __forceinline__ void load(const T* p, float (&o)[1]) { o[0] = Elem<T>::load(p, 0); }
};

// Branch-free stream access.  hipcc turns a per-element "load or zero" on a runtime condition into a branch around
// every load with an s_waitcnt vmcnt(0) behind it (fully serialised loads), so every load below is UNCONDITIONAL on
// a clamped, always-valid address and invalid lanes are zeroed with a select afterwards.  FAST (tile interior,
// rows aligned) uses one vector access; the generic form loads element-wise.
template <typename T, int N, bool FAST>
__device__ __forceinline__ void load_px(const T* rowp, int px, int P, float (&o)[N]) {
    if constexpr (FAST) {
        PixVec<T, N>::load(rowp + px, o);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int q = px + i;
            o[i] = Elem<T>::load(rowp, q < P ? q : P - 1) * ((q < P) ? 1.0f : 0.0f);
        }
    }
}
template <typename T, bool FAST>
__device__ __forceinline__ void store_px4(T* rowp, int px, int P, const float (&o)[4]) {
    if constexpr (FAST) {
        PixVec<T, 4>::store(rowp + px, o);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (px + i < P) Elem<T>::store(rowp, px + i, o[i]);
    }
}
// ---- buffer addressing for the aligned interior ------------------------------------------------------------- //
// 4 consecutive pixels of a 32-row batch block through raw buffer instructions: ONE per-lane byte offset (voffset)
// plus a wave-uniform row offset (soffset, an SGPR) per access, against a descriptor whose num_records ends at row
// B.  Compared with 64-bit flat addresses this frees the ~2 VGPRs per outstanding access that the 16 loads + 16
// stores of a block cost, and rows >= B need no branch: out-of-range loads return 0, out-of-range stores are dropped.
typedef __amdgpu_buffer_rsrc_t buf_rsrc;
// cache policy of the streaming buffer accesses (gfx950 aux bits: 1 = sc0, 2 = nt, 16 = sc1); tools/exp_cache_policy.sh
#ifndef ADIL_AUX_LD
#define ADIL_AUX_LD 0
#endif
#ifndef ADIL_AUX_ST
#define ADIL_AUX_ST 0
#endif
__device__ __forceinline__ buf_rsrc block_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
template <typename T> struct BufPx;
template <> struct BufPx<float> {
    typedef u32x4 Raw;
    static __device__ __forceinline__ Raw load(buf_rsrc r, int voff, int soff) {
        return __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, ADIL_AUX_LD);
    }
    static __device__ __forceinline__ void unpack(const Raw& t, float (&o)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = __uint_as_float(t[i]);
    }
    // buffer_store_dwordx4 + explicit wait states.  The hardware reads store data wider than 64 bits some cycles after
    // issue, and hipcc's hazard recogniser exempts MUBUF stores with an SGPR soffset from the wait state it inserts
    // for that.  Measured on gfx950 without the s_nop: under load the NEXT row's values (written to the same VGPRs
    // right after the store issues) land in memory.  The sched_barriers pin store -> s_nop -> next VALU write.
    static __device__ __forceinline__ void store(buf_rsrc r, int voff, int soff, const float (&o)[4]) {
        Raw t;
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = __float_as_uint(o[i]);
        __builtin_amdgcn_raw_buffer_store_b128(t, r, voff, soff, ADIL_AUX_ST);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 1");
        __builtin_amdgcn_sched_barrier(0);
    }
};
template <> struct BufPx<bf16_t> {
    typedef u32x2 Raw;
    static __device__ __forceinline__ Raw load(buf_rsrc r, int voff, int soff) {
        return __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, ADIL_AUX_LD);
    }
    static __device__ __forceinline__ void unpack(const Raw& t, float (&o)[4]) {
        o[0] = __uint_as_float(t[0] << 16); o[1] = __uint_as_float(t[0] & 0xffff0000u);
        o[2] = __uint_as_float(t[1] << 16); o[3] = __uint_as_float(t[1] & 0xffff0000u);
    }
    static __device__ __forceinline__ void store(buf_rsrc r, int voff, int soff, const float (&o)[4]) {
        Raw t;
        t[0] = pack2_bf16(o[0], o[1]);
        t[1] = pack2_bf16(o[2], o[3]);
        __builtin_amdgcn_raw_buffer_store_b64(t, r, voff, soff, ADIL_AUX_ST);
    }
};

// The x rows of adil_synth_store: row b of the batch is row index[b] of an R x P 8-bit image store, byte u standing for
// u8_unit(u) (looked up in a 256-entry LDS table).  R * P may exceed 4 GB, so a row's offset is formed in 64 bits and
// the bytes come through a global load, never through a 32-bit buffer offset.  4 consecutive pixels = one dword (P % 8
// == 0, the store 4-byte aligned); rows >= B read row B-1 (they are never stored).
struct StoreRows {
    const unsigned char* st;
    const int64_t* idx;
    const float* tab;
    int B, P;
    __device__ __forceinline__ unsigned raw4(int row, int px) const {
        const int64_t r = idx[row < B ? row : B - 1];
        return *reinterpret_cast<const unsigned*>(st + r * (int64_t)P + px);
    }
    __device__ __forceinline__ void unpack(unsigned t, float (&o)[4]) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = tab[(t >> (8 * i)) & 255u];
    }
    // the element-wise tiles: px may lie past the row end (a whole group of 4 does, P % 4 == 0) -> zeros
    __device__ __forceinline__ void load4(int row, int px, float (&o)[4]) const {
        unpack(raw4(row, px < P ? px : P - 4), o);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] *= (px < P) ? 1.0f : 0.0f;
    }
};

// 8 consecutive fp32 values (16-B aligned, e.g. a row of the packed codes) as an MFMA fragment
template <typename T>
__device__ __forceinline__ typename Mma<T>::Frag frag_from_f32x8(const float* p, float scale = 1.0f) {
    const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
    float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    if constexpr (Mma<T>::SCALED) {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] *= scale;
    }
    return Mma<T>::from8(f);
}

// Workgroup barrier for LDS hand-offs that leaves global loads in flight.  __syncthreads() carries a workgroup-scope
// fence that hipcc lowers to s_waitcnt vmcnt(0) before s_barrier, which drains the prefetched next-tile loads at every
// barrier (measured: no overlap of HBM with the LDS/MFMA phase).  Only LDS traffic has to be complete here.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

__device__ __forceinline__ int c_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// =========================================================================================================== //
// K1 (+K9) synthesis.  Workgroup = 4 waves = one 128-pixel slice of D (converted + staged once in LDS) swept
// over the whole batch; wave w takes batch blocks w, w+4, ...  Per 32x128 output block a wave issues 16 vector
// loads of x straight into the accumulators (C operand), Kp/16 k-groups of MFMAs against the LDS-resident D
// slice, and 16 vector stores.  Lane c of pixel tile t owns pixel p0 + 4c + t, so that one lane's four tiles
// are 4 CONSECUTIVE pixels: 16-byte (fp32) / 8-byte (bf16) accesses, 512 / 256 contiguous bytes per row.
// LDS row of pixel r: (r&3)*32 + (r>>2)  (tile-major), row stride Kp + PAD elements.
// =========================================================================================================== //
#define SYNTH_TILE 128

template <typename T, typename O, bool XACC, bool FAST, bool STORE = false>
__device__ __forceinline__ void synth_sweep(const T* __restrict__ x, const float* __restrict__ vp, T* __restrict__ out,
                                            const typename DImg<O>::Elem* sd, int B, int P, int Kp, int Ks, int p0,
                                            float delta_clamp, int pixel_clamp, int w, int c, int h, OpScale sc,
                                            StoreRows srows = {}) {
    using M = Mma<O>;
    using Frag = typename M::Frag;
    const int plane = SYNTH_TILE * Ks;
    const int NG = Kp >> 4;
    const int nbb = (B + 31) >> 5;
    const int px = p0 + 4 * c;
    const float xs = sc.v * sc.d;                 // scaled operands: x rides in the accumulator in product units
    for (int bb = w; bb < nbb; bb += 4) {
        const int b0 = bb << 5;
        f32x16 acc[4];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            float xv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (XACC) {
                const int row = b0 + c_row(reg, h);
                if constexpr (STORE) srows.load4(row, px, xv);
                else load_px<T, 4, FAST>(x + (size_t)(row < B ? row : B - 1) * P, px, P, xv);   // rows >= B are never stored
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t][reg] = M::SCALED ? xv[t] * xs : xv[t];
        }
        const float* arow = vp + (size_t)(b0 + c) * Kp + 8 * h;
        Frag a = frag_from_f32x8<O>(arow, sc.v);
        for (int g = 0; g < NG; ++g) {
            const int gn = (g + 1 < NG) ? g + 1 : g;
            const Frag an = frag_from_f32x8<O>(arow + 16 * gn, sc.v);                      // prefetch the next k-group
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const Frag bf = DImg<O>::load8(sd + (t * 32 + c) * Ks + 16 * g + 8 * h, plane);
                M::mma(acc[t], a, bf);
            }
            a = an;
        }
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = b0 + c_row(reg, h);
            float r[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) r[t] = M::SCALED ? acc[t][reg] * sc.o : acc[t][reg];
            if (!XACC) {
                if (delta_clamp >= 0.0f) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) r[t] = fminf(fmaxf(r[t], -delta_clamp), delta_clamp);
                }
                if (x != nullptr) {
                    float xv[4];
                    if constexpr (STORE) srows.load4(row, px, xv);
                    else load_px<T, 4, FAST>(x + (size_t)(row < B ? row : B - 1) * P, px, P, xv);
#pragma unroll
                    for (int t = 0; t < 4; ++t) r[t] += xv[t];
                }
            }
            if (pixel_clamp) {
#pragma unroll
                for (int t = 0; t < 4; ++t) r[t] = fminf(fmaxf(r[t], 0.0f), 1.0f);
            }
            if (row < B) store_px4<T, FAST>(out + (size_t)row * P, px, P, r);
        }
    }
}

template <typename T, bool XACC, bool PIXCLAMP, bool SCALED, bool STORE = false>
__device__ __forceinline__ void synth_store_buf(const f32x16 (&acc)[4], buf_rsrc rx, buf_rsrc ro, int voff, unsigned rowb,
                                                float delta_clamp, float oscale, const StoreRows& srows = {}, int row0 = 0,
                                                int px = 0) {
    using BP = BufPx<T>;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int soff = (int)((unsigned)c_row(reg, 0) * rowb);
        float r[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) r[t] = SCALED ? acc[t][reg] * oscale : acc[t][reg];
        if (!XACC) {
            if (delta_clamp >= 0.0f) {
#pragma unroll
                for (int t = 0; t < 4; ++t) r[t] = fminf(fmaxf(r[t], -delta_clamp), delta_clamp);
            }
            float xv[4];
            if constexpr (STORE) srows.unpack(srows.raw4(row0 + c_row(reg, 0), px), xv);
            else BP::unpack(BP::load(rx, voff, soff), xv);                                // x == NULL: empty buffer -> 0
#pragma unroll
            for (int t = 0; t < 4; ++t) r[t] += xv[t];
        }
        if (PIXCLAMP) {
#pragma unroll
            for (int t = 0; t < 4; ++t) r[t] = fminf(fmaxf(r[t], 0.0f), 1.0f);
        }
        BP::store(ro, voff, soff, r);
    }
}

// Aligned-interior sweep (FAST tiles): buffer addressing (see BufPx) and the code fragments of the first
// HOIST k-groups loaded up front, BEFORE the 16 x loads, so that per batch block a wave pays one L2 round trip
// for its codes (hidden under the HBM latency of x) instead of one per k-group in the MFMA loop.
// HOIST = 4 covers K <= 64; K > 64 runs the HOIST = 8 instantiation (all k-groups up front; costs ~45 registers, i.e. one
// resident workgroup per CU less, which the K <= 64 stream cannot afford)
// STORE: the x rows come from an 8-bit store (StoreRows) through global loads; out still goes through buffers.
template <typename T, typename O, bool XACC, int HOIST, int NWV = 4, bool STORE = false>
__device__ __forceinline__ void synth_sweep_buf(const T* __restrict__ x, const float* __restrict__ vp,
                                                T* __restrict__ out, const typename DImg<O>::Elem* sd, int B, int P,
                                                int Kp, int Ks, int p0, float delta_clamp, int pixel_clamp, int w, int c,
                                                int h, OpScale sc, StoreRows srows = {}) {
    using M = Mma<O>;
    using Frag = typename M::Frag;
    using BP = BufPx<T>;
    const int plane = SYNTH_TILE * Ks;
    const int NG = Kp >> 4;
    const int nbb = (B + 31) >> 5;
    const unsigned rowb = (unsigned)P * (unsigned)sizeof(T);
    const int voff = (int)((unsigned)(4 * h) * rowb) + (p0 + 4 * c) * (int)sizeof(T);
    for (int bb = w; bb < nbb; bb += NWV) {
        const int b0 = bb << 5;
        const int rows = B - b0 < 32 ? B - b0 : 32;
        const bool xbuf = !STORE && x;
        const buf_rsrc rx = block_rsrc(xbuf ? x + (size_t)b0 * P : nullptr, xbuf ? (unsigned)rows * rowb : 0u);
        const buf_rsrc ro = block_rsrc(out + (size_t)b0 * P, (unsigned)rows * rowb);
        typename std::conditional<STORE, unsigned, typename BP::Raw>::type xr[16];
        if (XACC) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                if constexpr (STORE) xr[reg] = srows.raw4(b0 + 4 * h + c_row(reg, 0), p0 + 4 * c);
                else xr[reg] = BP::load(rx, voff, (int)((unsigned)c_row(reg, 0) * rowb));
            }
        }
        const float* arow = vp + (size_t)(b0 + c) * Kp + 8 * h;
        float4 araw[HOIST][2];
#pragma unroll
        for (int g = 0; g < HOIST; ++g) {
            const float* ap = arow + 16 * (g < NG ? g : NG - 1);
            araw[g][0] = *reinterpret_cast<const float4*>(ap);
            araw[g][1] = *reinterpret_cast<const float4*>(ap + 4);
        }
        // All loads of the block are in flight before anything is consumed.  Left alone, hipcc sinks the code loads
        // (and their conversion) into the `g < NG` blocks next to their MFMAs: one exposed L2 round trip per k-group.
        // The opaque uses below pin them here (the x loads were issued first, so nothing waits longer than it must).
        __builtin_amdgcn_sched_barrier(0);
        Frag a[HOIST];
#pragma unroll
        for (int g = 0; g < HOIST; ++g) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
                asm volatile("" : "+v"(araw[g][u].x), "+v"(araw[g][u].y), "+v"(araw[g][u].z), "+v"(araw[g][u].w));
            float f[8] = {araw[g][0].x, araw[g][0].y, araw[g][0].z, araw[g][0].w,
                          araw[g][1].x, araw[g][1].y, araw[g][1].z, araw[g][1].w};
            if constexpr (M::SCALED) {
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] *= sc.v;
            }
            a[g] = M::from8(f);
        }
        f32x16 acc[4];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            float xv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (XACC) {
                if constexpr (STORE) srows.unpack(xr[reg], xv);
                else BP::unpack(xr[reg], xv);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t][reg] = M::SCALED ? xv[t] * (sc.v * sc.d) : xv[t];
        }
#pragma unroll
        for (int g = 0; g < HOIST; ++g) {
            if (g < NG) {
#pragma unroll
                for (int t = 0; t < 4; ++t) M::mma(acc[t], a[g], DImg<O>::load8(sd + (t * 32 + c) * Ks + 16 * g + 8 * h, plane));
            }
        }
        for (int g = HOIST; g < NG; ++g) {                                         // K > 64
            const Frag ag = frag_from_f32x8<O>(arow + 16 * g, sc.v);
#pragma unroll
            for (int t = 0; t < 4; ++t) M::mma(acc[t], ag, DImg<O>::load8(sd + (t * 32 + c) * Ks + 16 * g + 8 * h, plane));
        }
        if (pixel_clamp)                                                                  // uniform: one branch per block
            synth_store_buf<T, XACC, true, M::SCALED, STORE>(acc, rx, ro, voff, rowb, delta_clamp, sc.o, srows, b0 + 4 * h,
                                                             p0 + 4 * c);
        else
            synth_store_buf<T, XACC, false, M::SCALED, STORE>(acc, rx, ro, voff, rowb, delta_clamp, sc.o, srows, b0 + 4 * h,
                                                              p0 + 4 * c);
    }
}

// The 128-pixel slice of the dictionary operand (D for synth, D_dagger^T for the z-step) -> LDS planes of DImg<T>,
// tile-major rows (pixel r at row (r&3)*32 + (r>>2)), padded atoms zeroed.  256 threads.
template <typename T, bool FAST, int NT = 256>
__device__ __forceinline__ void fill_dict_slice(const float* __restrict__ d, typename DImg<T>::Elem* sd, int p0, int P, int K,
                                                int Kp, int Ks, int tid, float dscale = 1.0f) {
    using DI = DImg<T>;
    using M = Mma<T>;
    const int plane = SYNTH_TILE * Ks;
    if constexpr (FAST) {
        // D slice -> LDS.  The slice (128 pixels x K atoms) is one contiguous, 16-byte aligned run of 32*K float4:
        // every thread issues up to 8 independent 16-byte loads before the first conversion, so the fill costs ONE
        // memory round trip for K <= 64 (a scalar-load loop pays one per 8 elements and keeps the workgroup's wave
        // slots idle for a third of its life).
        const float4* src = reinterpret_cast<const float4*>(d + (size_t)p0 * K);
        const int nq = 32 * K;
        const float rk = 1.0f / (float)K;
        for (int q0 = tid; q0 < nq; q0 += NT * 8) {
            float4 val[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + NT * u;
                val[u] = src[q < nq ? q : nq - 1];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + NT * u;
                if (q < nq) {
                    const int i = 4 * q;
                    int r = (int)(((float)i + 0.5f) * rk);           // i / K, exact: |error| << 0.5 / K for i < 2^14
                    int k = i - r * K;
                    float e4[4] = {val[u].x, val[u].y, val[u].z, val[u].w};
                    if constexpr (M::SCALED) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) e4[e] *= dscale;
                    }
                    if ((K & 3) == 0) {                              // uniform: the quad stays inside one row
                        DI::put4(sd, ((r & 3) * 32 + (r >> 2)) * Ks + k, plane, e4);
                    } else if ((K & 1) == 0) {                       // pairs stay inside one row
                        const float lo[2] = {e4[0], e4[1]}, hi[2] = {e4[2], e4[3]};
                        DI::put2(sd, ((r & 3) * 32 + (r >> 2)) * Ks + k, plane, lo);
                        k += 2;
                        if (k == K) { k = 0; ++r; }
                        DI::put2(sd, ((r & 3) * 32 + (r >> 2)) * Ks + k, plane, hi);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            DI::put(sd, ((r & 3) * 32 + (r >> 2)) * Ks + k, plane, e4[e]);
                            if (++k == K) { k = 0; ++r; }
                        }
                    }
                }
            }
        }
        if (NT == 256 || tid < 256)
        for (int k = K + (tid & 1); k < Kp; k += 2)                   // zero the padded atoms of row tid/2
            DI::put(sd, (((tid >> 1) & 3) * 32 + (tid >> 3)) * Ks + k, plane, 0.0f);
    } else {
        // element-wise fill with pixel / atom guards: eight independent loads are issued before the first conversion
        for (int i0 = tid; i0 < SYNTH_TILE * Kp; i0 += NT * 8) {
            float val[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + NT * u;
                const int r = i / Kp, k = i - r * Kp;
                const int p = p0 + r;
                const float ok = ((p < P) && (k < K)) ? 1.0f : 0.0f;
                val[u] = d[(size_t)(p < P ? p : P - 1) * K + (k < K ? k : K - 1)] * ok;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + NT * u;
                const int r = i / Kp, k = i - r * Kp;
                DI::put(sd, ((r & 3) * 32 + (r >> 2)) * Ks + k, plane, M::SCALED ? val[u] * dscale : val[u]);
            }
        }
    }
}

// The 128-pixel slice of a dictionary that is ALREADY fp8 (the persistent e4m3 copy adil_adamw_clamp_fp8 maintains,
// bytes = e4m3(256 d), P x K row-major): one contiguous run of 128 K bytes, copied dword-wise into the tile-major LDS rows
// (K % 4 == 0, so a dword never straddles two pixels; row stride Ks is a multiple of 8).  A quarter of the bytes the fp32
// master costs, and no conversion work.
template <int NT>
__device__ __forceinline__ void fill_dict_slice_fp8(const unsigned char* __restrict__ d8, unsigned char* sd, int p0, int K, int Kp,
                                                    int Ks, int tid) {
    const unsigned* src = reinterpret_cast<const unsigned*>(d8 + (size_t)p0 * K);
    const int nq = 32 * K;                                        // dwords of the slice
    const float rk = 1.0f / (float)K;
    for (int q0 = tid; q0 < nq; q0 += NT * 8) {
        unsigned val[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = q0 + NT * u;
            val[u] = src[q < nq ? q : nq - 1];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = q0 + NT * u;
            if (q < nq) {
                const int i = 4 * q;
                const int r = (int)(((float)i + 0.5f) * rk);      // i / K (exact, see fill_dict_slice)
                const int k = i - r * K;
                *reinterpret_cast<unsigned*>(sd + ((r & 3) * 32 + (r >> 2)) * Ks + k) = val[u];
            }
        }
    }
    if (NT == 256 || tid < 256)
        for (int k = K + (tid & 1); k < Kp; k += 2) sd[(((tid >> 1) & 3) * 32 + (tid >> 3)) * Ks + k] = 0;   // e4m3 0x00 = +0
}

// STORE (adil_synth_store): `x` is the 8-bit image store (bytes, R x P) and `xidx` the batch's B rows of it; the 256-entry
// value table sits in LDS behind the D planes.
template <typename T, typename O, bool XACC, bool FAST, int HOIST = 4, int NWV = 4, bool PACKED = false, bool STORE = false>
__global__ __launch_bounds__(NWV * 64) __attribute__((amdgpu_waves_per_eu(NWV == 4 ? 3 : 2))) void synth_mfma_kernel(const T* __restrict__ x, const float* __restrict__ d,
                                                         const float* __restrict__ vp, T* __restrict__ out, int B,
                                                         int P, int K, int Kp, float delta_clamp, int pixel_clamp,
                                                         int tile0, OpScale sc, const int64_t* __restrict__ xidx = nullptr) {
    using DE = typename DImg<O>::Elem;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    DE* sd = reinterpret_cast<DE*>(smem_raw);                    // [PLANES][128][Ks] bf16 (fp8: bytes)
    const int Ks = Kp + DPAD;
    const int plane = SYNTH_TILE * Ks;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    // consecutive tiles go to consecutive workgroups, i.e. round-robin over the 8 XCDs: for this pure stream that is
    // 8 % faster than giving each XCD one contiguous range of tiles (measured)
    const int p0 = (tile0 + blockIdx.x) * SYNTH_TILE;
    if constexpr (PACKED)                                         // `d` is the fp8 copy (bytes), not the fp32 master
        fill_dict_slice_fp8<NWV * 64>(reinterpret_cast<const unsigned char*>(d), reinterpret_cast<unsigned char*>(sd), p0, K, Kp, Ks, tid);
    else
        fill_dict_slice<O, FAST, NWV * 64>(d, sd, p0, P, K, Kp, Ks, tid, sc.d);
    StoreRows srows = {};
    if constexpr (STORE) {
        float* tab = reinterpret_cast<float*>(smem_raw + (size_t)DImg<O>::PLANES * plane * sizeof(DE));
        if (tid < 256) tab[tid] = u8_unit(tid);
        srows = StoreRows{reinterpret_cast<const unsigned char*>(x), xidx, tab, B, P};
    }
    __syncthreads();
    if constexpr (FAST)
        synth_sweep_buf<T, O, XACC, HOIST, NWV, STORE>(x, vp, out, sd, B, P, Kp, Ks, p0, delta_clamp, pixel_clamp,
                                    __builtin_amdgcn_readfirstlane(w), c, h, sc, srows);
    else
        synth_sweep<T, O, XACC, FAST, STORE>(x, vp, out, sd, B, P, Kp, Ks, p0, delta_clamp, pixel_clamp, w, c, h, sc, srows);
}

// =========================================================================================================== //
// K8  fused inference step of forward_supervised_DDrague (adil.py:551-559):  the gradient wrt z,
//     gz = (dL/dv) D_dagger  (same contraction as the synthesis, vp := packed dL/dv, d := D_dagger^T),
// is formed in the MFMA accumulators and consumed on the spot by AdamW(z) + clamp(+-eps) + max|dz| — it is never
// written to HBM.  Same workgroup / fragment layout as synth_mfma_kernel; z, m, s are fp32 B x P.
// =========================================================================================================== //
// AdamW(z) + clamp + max|dz| on one 16-byte group of a row; gz = the matching accumulator entries
__device__ __forceinline__ float zstep_quad(float (&zv)[4], float (&mv)[4], float (&sv)[4], const f32x16 (&acc)[4], int reg,
                                            const AdamWHyper& hy, float lo, float hi) {
    float dmax = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float q = adamw_elem(zv[t], acc[t][reg], mv[t], sv[t], hy);
        q = fminf(fmaxf(q, lo), hi);
        dmax = fmaxf(dmax, fabsf(q - zv[t]));
        zv[t] = q;
    }
    return dmax;
}

template <bool FAST, int NWV = 4>
__global__ __launch_bounds__(NWV * 64) void zstep_mfma_kernel(float* __restrict__ z, float* __restrict__ m,
                                                         float* __restrict__ sq, const float* __restrict__ d,
                                                         const float* __restrict__ vp, int B, int P, int K, int Kp,
                                                         AdamWHyper hy, float lo, float hi, float* max_abs_delta,
                                                         int tile0, const float* skip_if_below, float skip_threshold,
                                                         float* clear, const float* __restrict__ dyn) {
    if (dyn != nullptr) { hy.step_size = dyn[0]; hy.bc2_sqrt = dyn[1]; }   // step-dependent scalars from device memory (graphs)
    using M = Mma<float>;
    using Frag = M::Frag;
    using DI = DImg<float>;
    using BP = BufPx<float>;
    // device-side stop test of the solver loop (adil.py:559): once the previous iteration's max|dz| fell below the
    // threshold every later launch is a no-op, so the host may look at the flag only every few iterations and still
    // return exactly the iterate the reference breaks at
    if (skip_if_below != nullptr && *skip_if_below < skip_threshold) {
        // stay stopped: this iteration's own slot reads 0 to the next launch, whatever an earlier round left in it
        if (max_abs_delta != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *max_abs_delta = 0.0f;
        return;
    }
    if (clear != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *clear = 0.0f;   // only one of the two range launches gets it
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sd = reinterpret_cast<bf16_t*>(smem_raw);            // [3][128][Ks] bf16: the h, m, l planes of D_dagger
    const int Ks = Kp + DPAD;
    const int plane = SYNTH_TILE * Ks;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int p0 = (tile0 + blockIdx.x) * SYNTH_TILE;
    fill_dict_slice<float, FAST, NWV * 64>(d, sd, p0, P, K, Kp, Ks, tid);
    __syncthreads();
    const int NG = Kp >> 4;
    const int nbb = (B + 31) >> 5;
    const int px = p0 + 4 * c;
    float dmax = 0.0f;
    if constexpr (FAST) {
        // Aligned interior: the six streams (z, m, s in and out) go through raw buffer instructions in groups of two
        // rows — 6 to 12 independent 16-byte loads per lane in flight, the next group requested before the current one
        // is consumed, the first group before the MFMA phase — so the kernel streams instead of paying one memory round
        // trip per row (round 1: 469 us for 1.88 GB).  Rows >= B: loads return 0, stores are dropped by the descriptor.
        const unsigned rowb = (unsigned)P * 4u;
        const int voff = (int)((unsigned)(4 * h) * rowb) + (p0 + 4 * c) * 4;
        for (int bb = __builtin_amdgcn_readfirstlane(w); bb < nbb; bb += NWV) {
            const int b0 = bb << 5;
            const int rows = B - b0 < 32 ? B - b0 : 32;
            const unsigned bytes = (unsigned)rows * rowb;
            const buf_rsrc rz = block_rsrc(z + (size_t)b0 * P, bytes), rm = block_rsrc(m + (size_t)b0 * P, bytes),
                           rs = block_rsrc(sq + (size_t)b0 * P, bytes);
            constexpr int GR = 2;                                // rows per group
            BP::Raw zr[2][GR], mr[2][GR], sr[2][GR];
#pragma unroll
            for (int j = 0; j < GR; ++j) {
                const int soff = (int)((unsigned)c_row(j, 0) * rowb);
                zr[0][j] = BP::load(rz, voff, soff); mr[0][j] = BP::load(rm, voff, soff); sr[0][j] = BP::load(rs, voff, soff);
            }
            f32x16 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
            const float* arow = vp + (size_t)(b0 + c) * Kp + 8 * h;
            Frag a = frag_from_f32x8<float>(arow);
            for (int g = 0; g < NG; ++g) {
                const int gn = (g + 1 < NG) ? g + 1 : g;
                const Frag an = frag_from_f32x8<float>(arow + 16 * gn);
#pragma unroll
                for (int t = 0; t < 4; ++t) M::mma(acc[t], a, DI::load8(sd + (t * 32 + c) * Ks + 16 * g + 8 * h, plane));
                a = an;
            }
#pragma unroll
            for (int grp = 0; grp < 16 / GR; ++grp) {
                const int cur = grp & 1, nxt = cur ^ 1;
                if (grp + 1 < 16 / GR) {
#pragma unroll
                    for (int j = 0; j < GR; ++j) {
                        const int soff = (int)((unsigned)c_row(GR * (grp + 1) + j, 0) * rowb);
                        zr[nxt][j] = BP::load(rz, voff, soff); mr[nxt][j] = BP::load(rm, voff, soff);
                        sr[nxt][j] = BP::load(rs, voff, soff);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);               // keep the next group's requests ahead of this group's use
#pragma unroll
                for (int j = 0; j < GR; ++j) {
                    const int reg = GR * grp + j;
                    const int soff = (int)((unsigned)c_row(reg, 0) * rowb);
                    float zv[4], mv[4], sv[4];
                    BP::unpack(zr[cur][j], zv); BP::unpack(mr[cur][j], mv); BP::unpack(sr[cur][j], sv);
                    dmax = fmaxf(dmax, zstep_quad(zv, mv, sv, acc, reg, hy, lo, hi));
                    BP::store(rz, voff, soff, zv); BP::store(rm, voff, soff, mv); BP::store(rs, voff, soff, sv);
                }
            }
        }
    } else {
        for (int bb = w; bb < nbb; bb += NWV) {
            const int b0 = bb << 5;
            f32x16 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
            const float* arow = vp + (size_t)(b0 + c) * Kp + 8 * h;
            for (int g = 0; g < NG; ++g) {
                const Frag a = frag_from_f32x8<float>(arow + 16 * g);
#pragma unroll
                for (int t = 0; t < 4; ++t) M::mma(acc[t], a, DI::load8(sd + (t * 32 + c) * Ks + 16 * g + 8 * h, plane));
            }
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = b0 + c_row(reg, h);
                const size_t ro = (size_t)(row < B ? row : B - 1) * P;        // rows >= B: valid address, never stored
                float zv[4], mv[4], sv[4];
                load_px<float, 4, false>(z + ro, px, P, zv);
                load_px<float, 4, false>(m + ro, px, P, mv);
                load_px<float, 4, false>(sq + ro, px, P, sv);
                const float zold[4] = {zv[0], zv[1], zv[2], zv[3]};
                (void)zstep_quad(zv, mv, sv, acc, reg, hy, lo, hi);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (row < B && px + t < P) dmax = fmaxf(dmax, fabsf(zv[t] - zold[t]));
                if (row < B) {
                    store_px4<float, false>(z + ro, px, P, zv);
                    store_px4<float, false>(m + ro, px, P, mv);
                    store_px4<float, false>(sq + ro, px, P, sv);
                }
            }
        }
    }
    if (max_abs_delta != nullptr) {
        dmax = wave_max(dmax);
        if (lane == 0 && dmax > 0.0f) atomic_max_nonneg(max_abs_delta, dmax);
    }
}

// =========================================================================================================== //
// K3  grad_d = g^T vp.  Each WAVE owns pixel tiles of PXT*32 pixels and sweeps all batch rows; the grad_d tile
// (PXT*32 px x AT*32 atoms) lives in the accumulators for the whole sweep.  A = g^T read in the coalesced
// "lane = PXT consecutive pixels, 8 batch rows per lane" layout (PXT*64 contiguous bytes per row and half-wave),
// B = codes from the transposed packed matrix vpt[atom][row] (L2 resident).  Waves are independent (no LDS).
// Rows >= B are read from a clamped (valid) row and multiply zero codes.
// =========================================================================================================== //
template <typename T, int PXT, int AT, bool FAST>
__global__ __launch_bounds__(256) void grad_d_mfma_kernel(const T* __restrict__ g,
                                                          const typename Mma<T>::Elem* __restrict__ vpt, int vstride,
                                                          float* __restrict__ grad_d, int B, int Bp, int P, int K,
                                                          int accumulate_d, int tile_begin, int tile_end) {
    using M = Mma<T>;
    using Frag = typename M::Frag;
    constexpr int TW = PXT * 32;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int tile = tile_begin + blockIdx.x * 4 + w;
    if (tile >= tile_end) return;                              // whole wave exits (no barriers in this kernel)
    const int p0 = tile * TW;
    const int px2 = p0 + PXT * c;
    f32x16 accd[PXT][AT];
#pragma unroll
    for (int t = 0; t < PXT; ++t)
#pragma unroll
        for (int at = 0; at < AT; ++at)
#pragma unroll
            for (int r = 0; r < 16; ++r) accd[t][at][r] = 0.0f;
    // 32 batch rows (two k-groups) per iteration: all 16 row loads are issued before the first MFMA needs them
    for (int b0 = 0; b0 < Bp; b0 += 32) {
        float raw[2][8][PXT];
#pragma unroll
        for (int g2 = 0; g2 < 2; ++g2)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int row = b0 + 16 * g2 + 8 * h + j;
                load_px<T, PXT, FAST>(g + (size_t)(row < B ? row : B - 1) * P, px2, P, raw[g2][j]);
            }
#pragma unroll
        for (int g2 = 0; g2 < 2; ++g2) {
            Frag afr[PXT];
#pragma unroll
            for (int t = 0; t < PXT; ++t) {
                float f[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = raw[g2][j][t];
                afr[t] = M::from8(f);
            }
#pragma unroll
            for (int at = 0; at < AT; ++at) {
                const Frag bfr = M::load8(vpt + (size_t)(at * 32 + c) * vstride + b0 + 16 * g2 + 8 * h);
#pragma unroll
                for (int t = 0; t < PXT; ++t) M::mma(accd[t][at], afr[t], bfr);
            }
        }
    }
    // epilogue: accumulator element (row i, lane c) of tile (t, at) is (pixel p0 + PXT*i + t, atom at*32 + c)
#pragma unroll
    for (int at = 0; at < AT; ++at) {
        const int atom = at * 32 + c;
        if (atom < K) {
            if (accumulate_d) {
#pragma unroll
                for (int t = 0; t < PXT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int pix = p0 + PXT * c_row(r, h) + t;
                        if (FAST || pix < P) grad_d[(size_t)pix * K + atom] += accd[t][at][r];
                    }
            } else {
#pragma unroll
                for (int t = 0; t < PXT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int pix = p0 + PXT * c_row(r, h) + t;
                        if (FAST || pix < P) grad_d[(size_t)pix * K + atom] = accd[t][at][r];
                    }
            }
        }
    }
}

// =========================================================================================================== //
// K2 / K6  grad_vb = g D  (also v = z D_dagger^T).  Workgroup = NW waves, wave w owns batch block w (32 rows) and
// keeps its 32 x AT*32 result in the accumulators while the workgroup walks a contiguous range of 64-pixel tiles:
//   * the D tile is converted and staged TRANSPOSED in LDS ([atom][pixel], double buffered, one barrier per tile)
//     and shared by all waves as the MFMA B operand;
//   * each wave streams its 32 x 64 block of g with fully coalesced 16-byte loads (8 or 4 rows of 128 / 256
//     contiguous bytes per instruction) into a wave-private LDS image and reads the A fragments (lane = batch row,
//     8 consecutive pixels) back with one ds_read_b128 per k-group; row strides are padded to an odd number of
//     16-byte slots, so both the writes and the reads are bank-conflict free.
// No atomics anywhere: partial sums leave through one slab per workgroup and a small reduction kernel, so the
// result is bitwise reproducible.  (A first version accumulated the partials with LDS float atomics:
// ds_add_f32 measured ~300 cycles per wave-instruction on gfx950 and made the kernel 6x slower.)
// =========================================================================================================== //
#define GV_TW 64

// D tile elements of one thread: consecutive threads -> consecutive atoms of one pixel (coalesced); the atom and
// pixel tails are zeroed by a multiply (never a select on the loaded value)
// (k0, kn): the atom window [k0, k0 + kn) this workgroup contracts against, of a dictionary with row stride K (the whole
// dictionary by default; one half of it when two workgroups split the atoms of a K > 64 dictionary, see grad_fused_mfma_kernel)
template <typename T, int AT, int NW, bool FAST>
__device__ __forceinline__ void gv_load_d(const float* __restrict__ d, int tile, int P, int K, int tid,
                                          float (&dreg)[(GV_TW * AT * 32 + NW * 64 - 1) / (NW * 64)], int k0 = 0, int kn = -1) {
    if (kn < 0) kn = K;
    // RAW loads only (clamped addresses).  The 0/1 tail mask is applied in gv_write_d, one phase later: any use of
    // these values here would make hipcc wait for them right away, and vmcnt being in issue order that wait also
    // drains every load issued before them (the prefetched g block).
    constexpr int KA = AT * 32, NT = NW * 64, DPT = (GV_TW * KA + NT - 1) / NT;
#pragma unroll
    for (int e = 0; e < DPT; ++e) {
        const int i = tid + e * NT;
        const int px = i / KA, a = i - px * KA;
        const int pix = tile * GV_TW + (px < GV_TW ? px : GV_TW - 1);
        dreg[e] = d[(size_t)((FAST || pix < P) ? pix : P - 1) * K + k0 + (a < kn ? a : kn - 1)];
    }
}
template <typename T, int AT, int NW, bool FAST>
__device__ __forceinline__ void gv_write_d(bf16_t* dst, int tile, int P, int K, int tid,
                                           const float (&dreg)[(GV_TW * AT * 32 + NW * 64 - 1) / (NW * 64)], int kn = -1) {
    constexpr int KA = AT * 32, NT = NW * 64, DPT = (GV_TW * KA + NT - 1) / NT, GD = GV_TW + DPAD;
    if (kn < 0) kn = K;
#pragma unroll
    for (int e = 0; e < DPT; ++e) {
        const int i = tid + e * NT;
        const int px = i / KA, a = i - px * KA;
        const int pix = tile * GV_TW + px;
        const float m = (a < kn && (FAST || pix < P)) ? 1.0f : 0.0f;   // atom / pixel tails: multiply, never a select
        if (px < GV_TW) DImg<T>::put(dst, a * GD + px, KA * GD, dreg[e] * m);
    }
}
// this wave's 32 x 64 block of g: NLD fully coalesced 16-byte loads per lane
template <typename T, bool FAST>
__device__ __forceinline__ void gv_load_g(const T* __restrict__ g, int tile, int b0, int B, int P, int lrow, int lcol,
                                          u32x4 (&blk)[32 / (64 / (GV_TW / (16 / (int)sizeof(T))))]) {
    constexpr int EPL = 16 / sizeof(T), LPR = GV_TW / EPL, RPI = 64 / LPR, NLD = 32 / RPI;
    const int p0 = tile * GV_TW;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int row = b0 + i * RPI + lrow;
        const T* rowp = g + (size_t)(row < B ? row : B - 1) * P;         // rows >= B: valid address, result discarded
        if constexpr (FAST) {
            blk[i] = *reinterpret_cast<const u32x4*>(rowp + p0 + lcol);
        } else {                                                  // ragged tail / unaligned rows: element-wise, clamped
            unsigned wds[4];                                      // (pixels beyond P meet zero rows of the D tile)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int q = p0 + lcol + e * (EPL / 4);
                if constexpr (sizeof(T) == 4) {
                    wds[e] = __float_as_uint(reinterpret_cast<const float*>(rowp)[q < P ? q : P - 1]);
                } else {
                    const unsigned lo = reinterpret_cast<const bf16_t*>(rowp)[q < P ? q : P - 1];
                    const unsigned hi = reinterpret_cast<const bf16_t*>(rowp)[q + 1 < P ? q + 1 : P - 1];
                    wds[e] = lo | (hi << 16);
                }
            }
            blk[i] = u32x4{wds[0], wds[1], wds[2], wds[3]};
        }
    }
}

template <typename T, int AT, int NW, bool FAST>
__global__ __launch_bounds__(NW * 64) void grad_v_mfma_kernel(const T* __restrict__ g, const float* __restrict__ d,
                                                              float* __restrict__ slab, int B, int Bp, int P, int K,
                                                              int tile_begin, int tile_end, int tiles_per_wg) {
    using M = Mma<T>;
    using E = typename M::Elem;
    using Frag = typename M::Frag;
    constexpr int KA = AT * 32;
    constexpr int GS = GV_TW + M::PAD;                       // row stride (elements): odd number of 16-B slots
    constexpr int EPL = 16 / sizeof(E);                          // elements per 16-byte lane access
    constexpr int LPR = GV_TW / EPL;                             // lanes per row of the g block
    constexpr int RPI = 64 / LPR;                                // rows per load instruction
    constexpr int NLD = 32 / RPI;                                // load instructions per 32-row block
    constexpr int NT = NW * 64;
    constexpr int DPT = (GV_TW * KA + NT - 1) / NT;              // D-tile elements per thread
    constexpr int GD = GV_TW + DPAD, DPL = KA * GD, DBUF = DImg<T>::PLANES * DPL;   // D tile: planes of [KA][GD] bf16
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sdt = reinterpret_cast<bf16_t*>(smem_raw);           // [2][PLANES][KA][GD]  transposed D tile, double buffered
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    E* sg = reinterpret_cast<E*>(sdt + 2 * DBUF) + (size_t)w * 32 * GS;   // this wave's [32][GS] image of its g block
    const int t0 = tile_begin + blockIdx.x * tiles_per_wg;
    const int t1 = min(tile_end, t0 + tiles_per_wg);
    const int b0 = w << 5;
    const bool active = b0 < Bp;                                 // waves beyond the batch only help staging D
    f32x16 accv[AT];
#pragma unroll
    for (int at = 0; at < AT; ++at)
#pragma unroll
        for (int r = 0; r < 16; ++r) accv[at][r] = 0.0f;
    const int lrow = lane / LPR, lcol = (lane - lrow * LPR) * EPL;

    float dreg[DPT];
    u32x4 blk[NLD];
    if (t0 < t1) {
        gv_load_d<T, AT, NW, FAST>(d, t0, P, K, tid, dreg);
        if (active) gv_load_g<T, FAST>(g, t0, b0, B, P, lrow, lcol, blk);
        gv_write_d<T, AT, NW, FAST>(sdt, t0, P, K, tid, dreg);
    }
    for (int tile = t0; tile < t1; ++tile) {
        const int buf = (tile - t0) & 1;
        const bool more = tile + 1 < t1;
        if (active) {
#pragma unroll
            for (int i = 0; i < NLD; ++i) *reinterpret_cast<u32x4*>(sg + (i * RPI + lrow) * GS + lcol) = blk[i];
        }
        if (more) {                                               // next tile's loads fly under this tile's MFMAs
            gv_load_d<T, AT, NW, FAST>(d, tile + 1, P, K, tid, dreg);
            if (active) gv_load_g<T, FAST>(g, tile + 1, b0, B, P, lrow, lcol, blk);
        }
        lds_barrier();                                          // D[buf] complete; everyone is done reading D[buf^1]
        if (active) {
            const bf16_t* sdb = sdt + buf * DBUF;
#pragma unroll
            for (int g3 = 0; g3 < GV_TW / 16; ++g3) {
                const Frag a = M::load8(sg + c * GS + 16 * g3 + 8 * h);
#pragma unroll
                for (int at = 0; at < AT; ++at) {
                    const Frag bfr = DImg<T>::load8(sdb + (at * 32 + c) * GD + 16 * g3 + 8 * h, DPL);
                    M::mma(accv[at], a, bfr);
                }
            }
        }
        if (more) gv_write_d<T, AT, NW, FAST>(sdt + (buf ^ 1) * DBUF, tile + 1, P, K, tid, dreg);
    }
    if (active) {                                                 // partial sums of this workgroup: slab[wg][row][atom < K]
        float* dst = slab + (size_t)blockIdx.x * Bp * K;
#pragma unroll
        for (int at = 0; at < AT; ++at)
            if (at * 32 + c < K) {
#pragma unroll
                for (int r = 0; r < 16; ++r) dst[(size_t)(b0 + c_row(r, h)) * K + at * 32 + c] = accv[at][r];
            }
    }
}

// =========================================================================================================== //
// K2 + K3 in ONE pass over g (the learning step needs both): the grad_v kernel above already parks the whole
// [NW*32 rows] x [64 px] block of g in LDS, so the grad_d tile of the same 64 pixels is formed from that image:
//   * the 64 px x AT*32 atoms tile is cut into 2*AT 32x32 MFMA tiles; wave w computes tile (w % (2*AT)) over the
//     row split (w / (2*AT)); its A fragments (lane = pixel, 8 consecutive batch rows) are COLUMN reads of the
//     images of the waves owning those rows: ds_read_b64_tr_b16 on the bf16 path (hardware transpose, 2 reads per
//     fragment), eight ds_read_b32 on the fp32 path; its B fragments (codes) are tile-invariant and live in
//     registers for the whole kernel;
//   * the KS = NW/(2*AT) row-split partials of a tile meet in LDS (fixed order) and each wave writes 16/KS registers
//     of the finished tile to grad_d.  Two barriers per 64-pixel tile.
// g is read from HBM exactly once; everything is bitwise reproducible.
// =========================================================================================================== //
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

template <typename T> struct ColFrag;
template <> struct ColFrag<bf16_t> {
    // lane (c = lane&31, h = lane>>5) receives rows rb+8h .. rb+8h+7 of column col0 + c of a [.][GS] bf16 image
    static __device__ __forceinline__ bf16x8 load(const bf16_t* img, int GS, int rb, int col0, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
        const int li = lane & 15, q = li >> 2, p = li & 3, gi = lane >> 4;
        const bf16_t* a = img + (rb + 8 * (gi >> 1) + q) * GS + col0 + 16 * (gi & 1) + 4 * p;
        typedef bf16x4 __attribute__((address_space(3))) * lds_ptr;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)a);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)(a + 4 * GS));
        return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#else
        return bf16x8{};
#endif
    }
};
template <> struct ColFrag<float> {
    static __device__ __forceinline__ Mma<float>::Frag load(const float* img, int GS, int rb, int col0, int lane) {
        float f[8];
        const float* a = img + (rb + 8 * (lane >> 5)) * GS + col0 + (lane & 31);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = a[j * GS];
        return Mma<float>::from8(f);
    }
};

template <typename T, int AT, int NW, int RB, bool FAST, bool ACC, bool WV = true>
__global__ __launch_bounds__(NW * 64) void grad_fused_mfma_kernel(const T* __restrict__ g, const float* __restrict__ d,
                                                                  const typename Mma<T>::Elem* __restrict__ vpt,
                                                                  int vstride, float* __restrict__ grad_d,
                                                                  float* __restrict__ slab, int B, int Bp, int P, int K,
                                                                  int tile_begin, int tile_end, int tiles_per_wg,
                                                                  int k_split, int nranges) {
    // k_split > 0 (K > 64 on AT = 2 tiles): TWO workgroups share a tile range and split the ATOMS — [0, k_split) and
    // [k_split, K) — instead of one workgroup holding all of them: a single workgroup with 128 atoms has room for 256 rows
    // only (its grad_v accumulators), which made a 512-row batch two passes over D and grad_d or two passes over g.  Each
    // half reads the whole g block (so g crosses the L2 twice) but only its own columns of D, writes its own columns of
    // grad_d and of the range's slab: D, grad_d and the slabs move once.  The halves of a range sit 8 block ids apart,
    // i.e. on the same XCD under the round-robin placement (speed only: the second reader of a g tile then finds it in
    // that XCD's L2 instead of fetching it from HBM again).
    int range = blockIdx.x, k0 = 0, kn = K;
    if (k_split > 0) {
        const int bid = blockIdx.x, half = (bid >> 3) & 1;
        range = (bid >> 4) * 8 + (bid & 7);
        if (range >= nranges) return;                             // whole workgroup, before any barrier
        k0 = half ? k_split : 0;
        kn = half ? K - k_split : k_split;
        // Both halves of a range walk its tiles in the SAME order: the second request for a g line then meets the first one
        // still in flight or fresh in the XCD's L2, and the two 200-byte halves of a grad_d row reach the L2 close enough
        // together to leave it as whole lines.  Counter traffic at 512 x 150528, K = 100: 301 MB = 1.10x algorithmic.  (Orders
        // that differ by a swap of neighbours — the halves then never wait for the same HBM round trip — were tried first and
        // measured 341 MB = 1.25x: a quarter of the second reads missed, and 15 MB of half-written lines were evicted and
        // fetched back; 3 % slower.  tools/exp/ablate_grad_fused.hip, profiles/r04_grad_fused_ablation.md.)
    }
    // WV = false: the grad_d half alone (no D tile, no grad_v accumulators, no slab) — the LDS-staged grad_d kernel of
    // K > 64, where the direct-load kernel is left with 128-byte row pieces (FINDINGS.md 17) and the fused kernel with 256 rows.
    // NW waves, each owning RB consecutive 32-row batch blocks (RB = 2 keeps the 512-row workgroup at 8 waves, i.e.
    // a 256-register budget per wave: with 16 waves the 128-register cap spills, and a scratch reload behind the
    // prefetched loads drains vmcnt and serialises the stream).
    using M = Mma<T>;
    using E = typename M::Elem;
    using Frag = typename M::Frag;
    constexpr int KA = AT * 32;
    constexpr int GS = GV_TW + M::PAD;
    constexpr int EPL = 16 / sizeof(E), LPR = GV_TW / EPL, RPI = 64 / LPR, NLD = 32 / RPI;
    constexpr int NT = NW * 64;
    constexpr int DPT = (GV_TW * KA + NT - 1) / NT;
    constexpr int NBLK = NW * RB;                                // 32-row blocks (= LDS images) per workgroup
    constexpr int NTILE = 2 * AT;                                // 32x32 MFMA tiles of the 64 px x KA grad_d tile
    static_assert(NW % NTILE == 0, "waves must split evenly over the grad_d tiles");
    constexpr int KS = NW / NTILE;                               // row splits per tile
    constexpr int RS = NBLK * 32 / KS;                           // rows per split
    constexpr int NKG = RS / 16;                                 // k-groups of 16 rows per wave
    constexpr int RPW = 16 / KS;                                 // accumulator registers each wave finishes
    static_assert(KS <= 16 && 16 % KS == 0, "row splits must divide the 16 accumulator registers");
    constexpr int GD = GV_TW + DPAD, DPL = KA * GD, DBUF = DImg<T>::PLANES * DPL;   // D tile: planes of [KA][GD] bf16
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sdt = reinterpret_cast<bf16_t*>(smem_raw);           // [2][PLANES][KA][GD]
    E* simg = reinterpret_cast<E*>(sdt + (WV ? 2 * DBUF : 0));   // [NBLK][32][GS]  the g block of this tile
    float* red = reinterpret_cast<float*>(simg + NBLK * 32 * GS);   // [NW][16][64]  grad_d row-split partials
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int t0 = tile_begin + range * tiles_per_wg;
    const int t1 = min(tile_end, t0 + tiles_per_wg);
    const int nt = t1 - t0;                                      // tiles of this range
    auto tile_at = [&](int i) __attribute__((always_inline)) { return t0 + i; };
    const int ti = w % NTILE, ks = w / NTILE, tp = ti & 1, ta = ti >> 1;

    f32x16 accv[WV ? RB : 1][WV ? AT : 1];
    if constexpr (WV) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int at = 0; at < AT; ++at)
#pragma unroll
                for (int r = 0; r < 16; ++r) accv[rb][at][r] = 0.0f;
    }
    const int lrow = lane / LPR, lcol = (lane - lrow * LPR) * EPL;

    // tile-invariant B fragments of grad_d: codes (transposed, converted) of this wave's row split
    typename M::Raw vfr[NKG];
#pragma unroll
    for (int kg = 0; kg < NKG; ++kg) {
        const int r0 = ks * RS + 16 * kg;
        const int rr = (r0 < Bp) ? r0 : 0;                       // splits beyond the batch are skipped below
        vfr[kg] = M::load8_raw(vpt + (size_t)(k0 + ta * 32 + c) * vstride + rr + 8 * h);
    }
    // Retire these loads BEFORE the tile loop.  hipcc's waitcnt insertion is path-insensitive: if the fragments could
    // still be in flight at the loop header it guards every use inside the loop with a counted vmcnt that, in steady
    // state, drains the prefetched next-tile loads instead (vmcnt is in issue order) — the kernel loses all overlap.
#pragma unroll
    for (int kg = 0; kg < NKG; ++kg) M::touch_raw(vfr[kg]);

    float dreg[DPT];
    u32x4 blk[RB][NLD];
    if (nt > 0) {
        const int tf = tile_at(0);
        if constexpr (WV) gv_load_d<T, AT, NW, FAST>(d, tf, P, K, tid, dreg, k0, kn);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
            if ((w * RB + rb) * 32 < Bp) gv_load_g<T, FAST>(g, tf, (w * RB + rb) * 32, B, P, lrow, lcol, blk[rb]);
        if constexpr (WV) gv_write_d<T, AT, NW, FAST>(sdt, tf, P, K, tid, dreg, kn);
    }
    for (int ti_ = 0; ti_ < nt; ++ti_) {
        const int tile = tile_at(ti_), tnext = tile_at(ti_ + 1);
        const int buf = ti_ & 1;
        const bool more = ti_ + 1 < nt;
        const int p0 = tile * GV_TW;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            if ((w * RB + rb) * 32 < Bp) {
                E* sg = simg + (size_t)(w * RB + rb) * 32 * GS;
#pragma unroll
                for (int i = 0; i < NLD; ++i) *reinterpret_cast<u32x4*>(sg + (i * RPI + lrow) * GS + lcol) = blk[rb][i];
            }
        }
        // An accumulating launch (second row chunk) needs the old grad_d values of THIS tile at the end of the
        // iteration.  They are requested here, BEFORE the next tile's loads: vmcnt retires in issue order, so waiting for
        // them later leaves the younger prefetch in flight (loading them next to the store drained it every iteration).
        float dold[ACC ? RPW : 1];
        if constexpr (ACC) {
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) {
                const int reg = (KS > 1) ? ks * RPW + rr : rr;
                const int pix = p0 + tp * 32 + c_row(reg, h);
                const int atom = ta * 32 + c;
                dold[rr] = grad_d[(size_t)((FAST || pix < P) ? pix : P - 1) * K + k0 + (atom < kn ? atom : kn - 1)];
            }
        }
        if (more) {                                               // next tile's loads fly under this tile's MFMAs
            if constexpr (WV) gv_load_d<T, AT, NW, FAST>(d, tnext, P, K, tid, dreg, k0, kn);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
                if ((w * RB + rb) * 32 < Bp) gv_load_g<T, FAST>(g, tnext, (w * RB + rb) * 32, B, P, lrow, lcol, blk[rb]);
        }
        lds_barrier();                                          // all images + D[buf] visible
        if constexpr (WV) {                                       // ---- grad_v: rows of this wave, all 64 pixels
            const bf16_t* sdb = sdt + buf * DBUF;
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                if ((w * RB + rb) * 32 < Bp) {
                    const E* sg = simg + (size_t)(w * RB + rb) * 32 * GS;
#pragma unroll
                    for (int g3 = 0; g3 < GV_TW / 16; ++g3) {
                        const Frag a = M::load8(sg + c * GS + 16 * g3 + 8 * h);
#pragma unroll
                        for (int at = 0; at < AT; ++at) {
                            const Frag bfr = DImg<T>::load8(sdb + (at * 32 + c) * GD + 16 * g3 + 8 * h, DPL);
                            M::mma(accv[rb][at], a, bfr);
                        }
                    }
                }
            }
        }
        // ---- grad_d: tile (tp, ta), rows ks*RS .. +RS
        f32x16 accd;
#pragma unroll
        for (int r = 0; r < 16; ++r) accd[r] = 0.0f;
        if constexpr (sizeof(T) == 4) {                          // fp32: keep the (loop-invariant) three-way split of the
#pragma unroll                                                    // codes from being hoisted back into 12 registers each
            for (int kg = 0; kg < NKG; ++kg) M::touch_raw(vfr[kg]);
        }
        if (Bp == NBLK * 32) {                                    // full workgroup: no per-k-group conditions, so the
#pragma unroll                                                    // column reads of several k-groups are in flight together
            for (int kg = 0; kg < NKG; ++kg) {
                const int r0 = ks * RS + 16 * kg;
                const Frag a = ColFrag<T>::load(simg + (size_t)(r0 >> 5) * 32 * GS, GS, r0 & 16, tp * 32, lane);
                M::mma(accd, a, M::expand(vfr[kg]));
            }
        } else {
#pragma unroll
            for (int kg = 0; kg < NKG; ++kg) {
                const int r0 = ks * RS + 16 * kg;
                if (r0 < Bp) {                                    // wave-uniform
                    const Frag a = ColFrag<T>::load(simg + (size_t)(r0 >> 5) * 32 * GS, GS, r0 & 16, tp * 32, lane);
                    M::mma(accd, a, M::expand(vfr[kg]));
                }
            }
        }
        if (KS > 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) red[(w * 16 + r) * 64 + lane] = accd[r];
            lds_barrier();                                      // partials visible; all image reads done
        }
        {
            const int atom = ta * 32 + c;
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) {
                const int reg = (KS > 1) ? ks * RPW + rr : rr;
                float sum;
                if (KS > 1) {
                    sum = 0.0f;
#pragma unroll
                    for (int q = 0; q < KS; ++q) sum += red[((ti + NTILE * q) * 16 + reg) * 64 + lane];
                } else {
                    sum = accd[rr];
                }
                const int pix = p0 + tp * 32 + c_row(reg, h);
                if (atom < kn && (FAST || pix < P)) {
                    float* o = grad_d + (size_t)pix * K + k0 + atom;
                    if constexpr (ACC) *o = dold[rr] + sum; else *o = sum;   // old value prefetched at the top
                }
            }
        }
        if (KS == 1) lds_barrier();                             // image reads done before the next tile overwrites
        if constexpr (WV) {
            if (more) gv_write_d<T, AT, NW, FAST>(sdt + (buf ^ 1) * DBUF, tnext, P, K, tid, dreg, kn);
        }
    }
    if constexpr (WV) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int b0 = (w * RB + rb) * 32;
        if (b0 < Bp) {
            float* dst = slab + (size_t)range * Bp * K + k0;      // compact rows of K atoms: no padded columns cross HBM
#pragma unroll
            for (int at = 0; at < AT; ++at)
                if (at * 32 + c < kn) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) dst[(size_t)(b0 + c_row(r, h)) * K + at * 32 + c] = accv[rb][at][r];
                }
        }
    }
    }
}

// =========================================================================================================== //
// Fused single pass for fp32 streams (aligned interior).  The generic kernel above, instantiated for fp32, is bound by
// conversion work: every wave splits the fp32 image fragments it reads (row fragments for grad_v, column fragments
// for grad_d) and re-expands the code fragments on every tile — 880 VALU per wave and 64-pixel tile next to 96
// MFMAs (117 us per 256 rows against 50 + 56 us for the two single-output kernels).  Here every operand is split
// ONCE: the g tile when it is copied to LDS (three bf16 planes, like the D tile), the codes before the loop (32-pixel
// tiles need only four code fragments per wave, so their twelve-register split form fits).  All fragment loads are
// then plain / transposed bf16 LDS reads, exactly as in the bf16 kernel, three planes each.  32-pixel tiles, two
// tiles in flight in two register stages; 256 rows per launch (LDS: planes of 256 x 32 px = 60 KB + D 30 KB + 32 KB).
// =========================================================================================================== //
template <int AT, int NW, bool ACC, bool WV = true>
__global__ __launch_bounds__(NW * 64) void grad_fused_f32_kernel(const float* __restrict__ g, const float* __restrict__ d,
                                                                 const float* __restrict__ vpt, int vstride,
                                                                 float* __restrict__ grad_d, float* __restrict__ slab, int B,
                                                                 int Bp, int P, int K, int ntiles, int tiles_per_wg) {
    using M = Mma<float>;
    using Frag = M::Frag;
    constexpr int TW = 32, KA = AT * 32, NT = NW * 64;
    constexpr int GI = TW + DPAD;                                // image plane row stride (bf16 elements): 5 x 16 B
    constexpr int IPL = NW * 32 * GI;                            // one image plane: [NW*32 rows][GI]
    constexpr int GD = TW + DPAD, DPL = KA * GD, DBUF = 3 * DPL; // D tile: three planes of [KA][GD]
    constexpr int LPR = TW / 4, RPI = 64 / LPR, NLD = 32 / RPI;  // fp32 rows: 8 lanes x 16 B per row, 8 rows per load, 4 loads
    constexpr int DPT = (TW * KA + NT - 1) / NT;
    constexpr int NTILE = AT, KS = NW / NTILE, RS = NW * 32 / KS, NKG = RS / 16, RPW = 16 / KS;
    static_assert(NW % NTILE == 0 && KS > 1 && 16 % KS == 0, "row splits must divide the 16 accumulator registers");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sdt = reinterpret_cast<bf16_t*>(smem_raw);           // [2][3][KA][GD]
    bf16_t* simg = sdt + (WV ? 2 * DBUF : 0);                    // [3][NW*32][GI]   (WV = false: grad_d alone, no D tile)
    float* red = reinterpret_cast<float*>(simg + 3 * IPL);       // [NW][16][64]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int t0 = blockIdx.x * tiles_per_wg;
    const int t1 = min(ntiles, t0 + tiles_per_wg);
    const int ta = w % NTILE, ks = w / NTILE;
    const int b0 = w * 32;
    const bool active = b0 < Bp;
    const int lrow = lane / LPR, lcol = (lane - lrow * LPR) * 4;

    f32x16 accv[WV ? AT : 1];
    if constexpr (WV) {
#pragma unroll
        for (int at = 0; at < AT; ++at)
#pragma unroll
            for (int r = 0; r < 16; ++r) accv[at][r] = 0.0f;
    }

    Frag vfr[NKG];                                               // codes of this wave's row split, split once
#pragma unroll
    for (int kg = 0; kg < NKG; ++kg) {
        const int r0 = ks * RS + 16 * kg;
        vfr[kg] = M::load8(vpt + (size_t)(ta * 32 + c) * vstride + ((r0 < Bp) ? r0 : 0) + 8 * h);
    }
#pragma unroll
    for (int kg = 0; kg < NKG; ++kg) M::touch(vfr[kg]);          // retired before the loop (see the generic kernel)

    struct Stage { float dreg[WV ? DPT : 1]; u32x4 blk[NLD]; };
    auto load_stage = [&](Stage& st, int tile) __attribute__((always_inline)) {
        if constexpr (WV) {
#pragma unroll
            for (int e = 0; e < DPT; ++e) {                       // raw loads, clamped addresses (masked when written)
                const int i = tid + e * NT;
                const int px = i / KA, a = i - px * KA;
                st.dreg[e] = d[(size_t)(tile * TW + (px < TW ? px : TW - 1)) * K + (a < K ? a : K - 1)];
            }
        }
        if (active) {
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int row = b0 + i * RPI + lrow;
                st.blk[i] = *reinterpret_cast<const u32x4*>(g + (size_t)(row < B ? row : B - 1) * P + tile * TW + lcol);
            }
        }
    };
    auto write_d = [&](bf16_t* dst, const Stage& st) __attribute__((always_inline)) {
        if constexpr (WV) {
#pragma unroll
            for (int e = 0; e < DPT; ++e) {
                const int i = tid + e * NT;
                const int px = i / KA, a = i - px * KA;
                if (px < TW) DImg<float>::put(dst, a * GD + px, DPL, st.dreg[e] * ((a < K) ? 1.0f : 0.0f));
            }
        }
    };
    Stage sa, sb;
    if (t0 < t1) load_stage(sa, t0);
    if (t0 + 1 < t1) load_stage(sb, t0 + 1);
    if (t0 < t1) write_d(sdt, sa);

    auto tile_step = [&](int tile, int dbuf, Stage& cur, Stage& oth) __attribute__((always_inline)) {
        if (active) {                                             // this wave's 32 rows -> the three image planes
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const float f4[4] = {__uint_as_float(cur.blk[i][0]), __uint_as_float(cur.blk[i][1]),
                                     __uint_as_float(cur.blk[i][2]), __uint_as_float(cur.blk[i][3])};
                DImg<float>::put4(simg, (b0 + i * RPI + lrow) * GI + lcol, IPL, f4);
            }
        }
        float dold[ACC ? RPW : 1];
        if constexpr (ACC) {                                      // old grad_d of THIS tile, requested before the prefetch
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) {
                const int atom = ta * 32 + c;
                dold[rr] = grad_d[(size_t)(tile * TW + c_row(ks * RPW + rr, h)) * K + (atom < K ? atom : K - 1)];
            }
        }
        if (tile + 2 < t1) load_stage(cur, tile + 2);
        lds_barrier();                                          // all image planes + D[dbuf] visible
        if (WV && active) {                                       // ---- grad_v: rows of this wave, all 32 pixels
            const bf16_t* sdb = sdt + dbuf * DBUF;
#pragma unroll
            for (int g3 = 0; g3 < TW / 16; ++g3) {
                const Frag a = DImg<float>::load8(simg + (b0 + c) * GI + 16 * g3 + 8 * h, IPL);
#pragma unroll
                for (int at = 0; at < AT; ++at)
                    M::mma(accv[at], a, DImg<float>::load8(sdb + (at * 32 + c) * GD + 16 * g3 + 8 * h, DPL));
            }
        }
        f32x16 accd;                                              // ---- grad_d: atom tile ta, rows ks*RS .. +RS
#pragma unroll
        for (int r = 0; r < 16; ++r) accd[r] = 0.0f;
#pragma unroll
        for (int kg = 0; kg < NKG; ++kg) {
            const int r0 = ks * RS + 16 * kg;
            if (Bp == NW * 32 || r0 < Bp) {                       // wave-uniform
                Frag a;
                a.h = ColFrag<bf16_t>::load(simg + (size_t)(r0 & ~31) * GI, GI, r0 & 16, 0, lane);
                a.m = ColFrag<bf16_t>::load(simg + IPL + (size_t)(r0 & ~31) * GI, GI, r0 & 16, 0, lane);
                a.l = ColFrag<bf16_t>::load(simg + 2 * IPL + (size_t)(r0 & ~31) * GI, GI, r0 & 16, 0, lane);
                M::mma(accd, a, vfr[kg]);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(w * 16 + r) * 64 + lane] = accd[r];
        lds_barrier();                                          // partials visible; all image and D[dbuf] reads done
        {
            const int atom = ta * 32 + c;
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) {
                const int reg = ks * RPW + rr;
                float sum = 0.0f;
#pragma unroll
                for (int q = 0; q < KS; ++q) sum += red[((ta + NTILE * q) * 16 + reg) * 64 + lane];
                if (atom < K) {
                    float* o = grad_d + (size_t)(tile * TW + c_row(reg, h)) * K + atom;
                    if constexpr (ACC) *o = dold[rr] + sum; else *o = sum;
                }
            }
        }
        if (tile + 1 < t1) write_d(sdt + (dbuf ^ 1) * DBUF, oth);
    };
    for (int tile = t0; tile < t1; tile += 2) {
        tile_step(tile, 0, sa, sb);
        if (tile + 1 < t1) tile_step(tile + 1, 1, sb, sa);
    }
    if (WV && active) {
        float* dst = slab + (size_t)blockIdx.x * Bp * K;
#pragma unroll
        for (int at = 0; at < AT; ++at)
            if (at * 32 + c < K) {
#pragma unroll
                for (int r = 0; r < 16; ++r) dst[(size_t)(b0 + c_row(r, h)) * K + at * 32 + c] = accv[at][r];
            }
    }
}

// =========================================================================================================== //
// grad_v for fp32 streams (aligned interior): the forward contraction v = z D_dagger^T of the DDrague iteration (fp32 z)
// and dL/dv = g D of the fp32 parity path.  Same idea as grad_fused_f32_kernel: the stream operand is split into its
// three bf16 planes ONCE, when the wave copies its 32 x 32-pixel block to LDS (the generic kernel splits every fragment
// at load time and fits only 256 rows per launch); with 32-pixel tiles the planes of 512 rows fit (120 KB + 30 KB of D
// planes), so the whole batch is one launch: D_dagger read once, one slab per workgroup.  A wave only ever reads its own
// rows of the image, so the single barrier per tile is for the shared D tile.  Two tiles in flight in two register stages.
// =========================================================================================================== //
template <int AT, int NW>
__global__ __launch_bounds__(NW * 64) void grad_v_f32_kernel(const float* __restrict__ g, const float* __restrict__ d,
                                                             float* __restrict__ slab, int B, int Bp, int P, int K, int ntiles,
                                                             int tiles_per_wg, int k_split, int nranges) {
    // k_split > 0: two workgroups per tile range split the atoms, as in grad_fused_mfma_kernel (K > 64 on the AT = 2 shape:
    // 512 rows per launch, D read once, one slab per range with both halves' columns; the halves sit on one XCD)
    int range = blockIdx.x, k0 = 0, kn = K;
    if (k_split > 0) {
        const int bid = blockIdx.x, half = (bid >> 3) & 1;
        range = (bid >> 4) * 8 + (bid & 7);
        if (range >= nranges) return;                             // whole workgroup, before any barrier
        k0 = half ? k_split : 0;
        kn = half ? K - k_split : k_split;
    }
    // Round 4: the in-wave software pipeline of round 3's ablation (tools/exp/ablate_grad_v_f32.hip, pipe_kernel: bit-identical
    // slabs, never slower on six boxes, mean -5 %): ONE register stage; a wave reads all A fragments of tile t first, then
    // the split + ds_write of tile t+1 — into the image rows it has just read, which only this wave ever reads — is
    // interleaved with the MFMAs of tile t (pinned with sched_barrier: the compiler's own schedule spills), and the loads
    // of tile t+2 are issued as the registers free up.  Tiles beyond the range are clamped loads against a zeroed D tile.
    using M = Mma<float>;
    using Frag = M::Frag;
    constexpr int TW = 32, KA = AT * 32, NT = NW * 64;
    constexpr int GI = TW + DPAD, IPL = NW * 32 * GI;            // image planes [3][NW*32][GI]
    constexpr int GD = TW + DPAD, DPL = KA * GD, DBUF = 3 * DPL; // D tile planes [2][3][KA][GD]
    constexpr int LPR = TW / 4, RPI = 64 / LPR, NLD = 32 / RPI;
    constexpr int DPT = (TW * KA + NT - 1) / NT;
    constexpr int NGRP = (TW / 16) * AT;                         // MFMA groups per tile (six MFMAs each)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sdt = reinterpret_cast<bf16_t*>(smem_raw);
    bf16_t* simg = sdt + 2 * DBUF;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int t0 = range * tiles_per_wg;
    const int t1 = min(ntiles, t0 + tiles_per_wg);
    const int tlast = max(t1 - 1, 0);
    const int b0 = w * 32;                                       // waves beyond the batch stream a clamped row: never stored
    const int lrow = lane / LPR, lcol = (lane - lrow * LPR) * 4;
    f32x16 accv[AT];
#pragma unroll
    for (int at = 0; at < AT; ++at)
#pragma unroll
        for (int r = 0; r < 16; ++r) accv[at][r] = 0.0f;
    float dreg[DPT];
    u32x4 blk[NLD];
    const float* grow[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int row = b0 + i * RPI + lrow;
        grow[i] = g + (size_t)(row < B ? row : B - 1) * P + lcol;
    }
    auto load_d = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < DPT; ++e) {
            const int i = tid + e * NT;
            const int px = i / KA, a = i - px * KA;
            dreg[e] = d[(size_t)(tile * TW + (px < TW ? px : TW - 1)) * K + k0 + (a < kn ? a : kn - 1)];
        }
    };
    auto load_img = [&](int i, int tile) __attribute__((always_inline)) {
        blk[i] = *reinterpret_cast<const u32x4*>(grow[i] + tile * TW);
    };
    auto split_img = [&](int i) __attribute__((always_inline)) {
        const float f4[4] = {__uint_as_float(blk[i][0]), __uint_as_float(blk[i][1]), __uint_as_float(blk[i][2]),
                             __uint_as_float(blk[i][3])};
        DImg<float>::put4(simg, (b0 + i * RPI + lrow) * GI + lcol, IPL, f4);
    };
    auto write_d = [&](bf16_t* dst, float valid) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < DPT; ++e) {
            const int i = tid + e * NT;
            const int px = i / KA, a = i - px * KA;
            if (px < TW) DImg<float>::put(dst, a * GD + px, DPL, dreg[e] * ((a < kn) ? valid : 0.0f));
        }
    };
    load_d(min(t0, tlast));
#pragma unroll
    for (int i = 0; i < NLD; ++i) load_img(i, min(t0, tlast));
    write_d(sdt, t0 < t1 ? 1.0f : 0.0f);
#pragma unroll
    for (int i = 0; i < NLD; ++i) split_img(i);
    load_d(min(t0 + 1, tlast));
#pragma unroll
    for (int i = 0; i < NLD; ++i) load_img(i, min(t0 + 1, tlast));

    auto tile_step = [&](int tile, int dbuf) __attribute__((always_inline)) {
        lds_barrier();                                          // D[dbuf] staged by everyone; everyone is done reading D[dbuf^1]
        const bf16_t* sdb = sdt + dbuf * DBUF;
        Frag a[TW / 16];
#pragma unroll
        for (int g3 = 0; g3 < TW / 16; ++g3) a[g3] = DImg<float>::load8(simg + (b0 + c) * GI + 16 * g3 + 8 * h, IPL);
        const int tnext = min(tile + 2, tlast);
        const float valid = tile + 1 < t1 ? 1.0f : 0.0f;
#pragma unroll
        for (int q = 0; q < NGRP; ++q) {
            const int g3 = q / AT, at = q - g3 * AT;
            M::mma(accv[at], a[g3], DImg<float>::load8(sdb + (at * 32 + c) * GD + 16 * g3 + 8 * h, DPL));
            // the LDS executes a wave's instructions in order: these writes land after the reads of a[] above
#pragma unroll
            for (int i = q * NLD / NGRP; i < (q + 1) * NLD / NGRP; ++i) {
                split_img(i);
                load_img(i, tnext);
            }
            if (q == NGRP - 1) {
                write_d(sdt + (dbuf ^ 1) * DBUF, valid);
                load_d(tnext);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    for (int tile = t0; tile < t1; tile += 2) {
        tile_step(tile, 0);
        tile_step(tile + 1, 1);                                   // an odd range's last step meets a zeroed D tile
    }
    if (b0 < Bp) {
        float* dst = slab + (size_t)range * Bp * K + k0;
#pragma unroll
        for (int at = 0; at < AT; ++at)
            if (at * 32 + c < kn) {
#pragma unroll
                for (int r = 0; r < 16; ++r) dst[(size_t)(b0 + c_row(r, h)) * K + at * 32 + c] = accv[at][r];
            }
    }
}

// =========================================================================================================== //
// K8 + K6 in one pass: the z-step above AND the codes of the NEXT DDrague iteration, v' = z_new D_dagger^T
// (adil.py:542 recomputes them from the z that adil.py:554-555 just wrote).  The z-step holds the freshly updated z tile
// in registers and the D_dagger slice of the same 128 pixels in LDS, so the separate contraction launch — its re-read of
// z (B P 4 bytes: 308 MB at 512 images) and of D_dagger — disappears from the loop.
//
// The contraction reduces over PIXELS, so its result is a sum over all slices: a workgroup therefore owns fixed ROWS
// (8 waves x RB blocks of 32) and WALKS a contiguous range of slices with the (32 rows x AT*32 atoms) accumulators of its
// blocks resident across the range, like grad_v_f32_kernel; it leaves one slab of partial sums per workgroup, summed by
// adil_pack_codes in the fixed slab_sum order (bitwise reproducible, no atomics).  Rows beyond one workgroup's
// 256 RB go to blockIdx.y and land in the same slab (disjoint rows), so the slab layout is [gridDim.x][Bp][K] for any B.
//
// MFMA operands of the new contraction: z_new sits in the C layout of the gz tiles (lane = pixel quad, registers = rows)
// and is needed in the A layout (lane = row, 8 consecutive reduction indices), i.e. transposed: each wave passes it
// through a private fp32 LDS image of 16 rows x 128 columns — half a block at a time, which is what fits next to the
// D_dagger planes — and contracts each half on the 16-row shape v_mfma_f32_16x16x32_bf16 (a first version put the half
// into 16 lanes of a 32 x 32 x 16 A operand and zeros into the other 16: twice the matrix work, paid at K = 100).
// Image column j = t*32 + c holds pixel 4c + t — the row order of the LDS slice — so that a k-group of 32 image columns
// meets 32 consecutive LDS rows of the slice, which come out as the B fragment (lane = atom, 8 consecutive pixels) of a
// transposing read (ds_read_b64_tr_b16, two per plane and fragment) — the same planes the gz contraction reads row-wise.
// z fragments are split into their three bf16 pieces after the read (each element is read exactly once).
// =========================================================================================================== //
#define ZC_IS 132                                               // image row stride (floats): 128 + 4, rows shift by 4 banks
// LDS row stride of the D_dagger planes is a COMPILE-TIME constant here (atoms padded to the tile count's maximum that
// still fits: 32, 64, 112): with a run-time stride hipcc keeps one address register per (k-group, plane) of the
// transposing reads — ~50 VGPRs of loop invariants, and the kernel spilled.
template <int AT> struct ZCodes { static constexpr int KP = AT == 4 ? 112 : AT * 32, KS = KP + DPAD; };

// v_mfma_f32_16x16x32_bf16 operands (layout as in adil_stem.hip, checked on hardware): A lane l -> row l&15, reduction
// indices 8*(l>>4)+j; B lane l -> column l&15, the same indices; C register r of lane l -> row 4*(l>>4)+r, column l&15.
typedef float f32x4v __attribute__((ext_vector_type(4)));
// B fragment as a transposing read of a [.][GS] bf16 image: lane (li = l&15, gi = l>>4) receives rows rb+8gi .. +7 of
// column col0 + li (each 16-lane group transposes the 4 x 16 block its lanes address, twice)
__device__ __forceinline__ bf16x8 colfrag16(const bf16_t* img, int GS, int rb, int col0, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int li = lane & 15, gi = lane >> 4;
    const bf16_t* a = img + (rb + 8 * gi + (li >> 2)) * GS + col0 + 4 * (li & 3);
    typedef bf16x4 __attribute__((address_space(3))) * lds_ptr;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)a);
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)(a + 4 * GS));
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#else
    return bf16x8{};
#endif
}
// the six-piece fp32-grade product of Mma<float>::mma on the 16 x 16 shape (same order: small terms first)
__device__ __forceinline__ void mma16_split(f32x4v& acc, const Mma<float>::Frag& a, const Mma<float>::Frag& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.l, b.h, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.l, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.m, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.h, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.m, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.h, acc, 0, 0, 0);
}

template <int AT, int RB>
__global__ __launch_bounds__(512) void zstep_codes_kernel(float* __restrict__ z, float* __restrict__ m,
                                                         float* __restrict__ sq, const float* __restrict__ d,
                                                         const float* __restrict__ vp, float* __restrict__ slab, int B,
                                                         int Bp, int P, int K, int Kp, AdamWHyper hy, float lo, float hi,
                                                         float* max_abs_delta, int nslices, int spw,
                                                         const float* skip_if_below, float skip_threshold, float* clear,
                                                         const float* __restrict__ dyn) {
    if (dyn != nullptr) { hy.step_size = dyn[0]; hy.bc2_sqrt = dyn[1]; }
    using M = Mma<float>;
    using Frag = M::Frag;
    using DI = DImg<float>;
    using BP = BufPx<float>;
    constexpr int NWV = 8, KP = ZCodes<AT>::KP, Ks = ZCodes<AT>::KS, plane = SYNTH_TILE * Ks;
    const bool first = blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0;
    // device-side stop test, as in zstep_mfma_kernel.  A skipped launch leaves the slabs alone: they still hold the codes
    // of the converged z, which is what every later pack_codes (and the final synthesis) has to see.
    if (skip_if_below != nullptr && *skip_if_below < skip_threshold) {
        if (max_abs_delta != nullptr && first) *max_abs_delta = 0.0f;
        return;
    }
    if (clear != nullptr && first) *clear = 0.0f;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sd = reinterpret_cast<bf16_t*>(smem_raw);            // [3][128][Ks] bf16: the h, m, l planes of D_dagger
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* img = reinterpret_cast<float*>(sd + 3 * plane) + w * 16 * ZC_IS;      // this wave's [16][ZC_IS] image
    const int NG = Kp >> 4;                                       // k-groups of the packed codes (Kp <= KP)
    const int s0 = blockIdx.x * spw, s1 = min(nslices, s0 + spw);
    const int wrow0 = (blockIdx.y * NWV + w) * RB * 32;          // first row of this wave's RB blocks
    const unsigned rowb = (unsigned)P * 4u;

    // accv[0] = the accumulators of the block being processed, accv[1] = the other block's (RB = 2): the block loop stays
    // ROLLED and the two sets trade places after every block — unrolled, the per-block address invariants of the second
    // block were what no longer fitted the register file (reloaded from scratch at every block start).
    constexpr int NT16 = KP / 16;                                // 16-atom tiles of the code contraction
    f32x4v accv[RB][2][NT16];                                    // [block][half of the block's rows][atom tile]
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
            for (int nt = 0; nt < NT16; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) accv[rb][hf][nt][r] = 0.0f;
    float dmax = 0.0f;

    for (int s = s0; s < s1; ++s) {
        const int p0 = s * SYNTH_TILE;
        if (s > s0) __syncthreads();                              // everyone is done with the previous slice
        fill_dict_slice<float, true, NWV * 64>(d, sd, p0, P, K, KP, Ks, tid);
        __syncthreads();
        const int voff = (int)((unsigned)(4 * h) * rowb) + (p0 + 4 * c) * 4;
#pragma unroll 1
        for (int rb = 0; rb < RB; ++rb) {
            const int b0 = wrow0 + rb * 32;
            if (b0 < Bp) {                                        // wave-uniform; no barrier inside
                const int rows = B - b0 < 32 ? B - b0 : 32;
                const unsigned bytes = (unsigned)rows * rowb;
                const buf_rsrc rz = block_rsrc(z + (size_t)b0 * P, bytes), rm = block_rsrc(m + (size_t)b0 * P, bytes),
                               rs = block_rsrc(sq + (size_t)b0 * P, bytes);
                constexpr int GR = 2;                            // rows per group (see zstep_mfma_kernel)
                BP::Raw zr[2][GR], mr[2][GR], sr[2][GR];
#pragma unroll
                for (int j = 0; j < GR; ++j) {
                    const int soff = (int)((unsigned)c_row(j, 0) * rowb);
                    zr[0][j] = BP::load(rz, voff, soff); mr[0][j] = BP::load(rm, voff, soff); sr[0][j] = BP::load(rs, voff, soff);
                }
                f32x16 acc[4];                                    // gz = (dL/dv) D_dagger of this block and slice
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
                const float* arow = vp + (size_t)(b0 + c) * Kp + 8 * h;
                Frag a = frag_from_f32x8<float>(arow);
#pragma unroll
                for (int g = 0; g < KP / 16; ++g) {
                    if (g < NG) {                                 // uniform
                        const Frag an = frag_from_f32x8<float>(arow + 16 * ((g + 1 < NG) ? g + 1 : g));
#pragma unroll
                        for (int t = 0; t < 4; ++t) M::mma(acc[t], a, DI::load8(sd + (t * 32 + c) * Ks + 16 * g + 8 * h, plane));
                        a = an;
                    }
                }
#pragma unroll
                for (int grp = 0; grp < 16 / GR; ++grp) {
                    const int cur = grp & 1, nxt = cur ^ 1;
                    if (grp + 1 < 16 / GR) {
#pragma unroll
                        for (int j = 0; j < GR; ++j) {
                            const int soff = (int)((unsigned)c_row(GR * (grp + 1) + j, 0) * rowb);
                            zr[nxt][j] = BP::load(rz, voff, soff); mr[nxt][j] = BP::load(rm, voff, soff);
                            sr[nxt][j] = BP::load(rs, voff, soff);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);           // keep the next group's requests ahead of this group's use
#pragma unroll
                    for (int j = 0; j < GR; ++j) {
                        const int reg = GR * grp + j;
                        const int soff = (int)((unsigned)c_row(reg, 0) * rowb);
                        float zv[4], mv[4], sv[4];
                        BP::unpack(zr[cur][j], zv); BP::unpack(mr[cur][j], mv); BP::unpack(sr[cur][j], sv);
                        dmax = fmaxf(dmax, zstep_quad(zv, mv, sv, acc, reg, hy, lo, hi));
                        BP::store(rz, voff, soff, zv); BP::store(rm, voff, soff, mv); BP::store(rs, voff, soff, sv);
                        float* irow = img + (c_row(reg, h) & 15) * ZC_IS + c;    // z_new -> image row of its half, column t*32 + c
#pragma unroll
                        for (int t = 0; t < 4; ++t) irow[t * 32] = zv[t];
                    }
                    if ((grp & 3) == 3) {
                        // rows 16*hf .. 16*hf+15 of the block are complete in the image: v' += z_new D_dagger^T for them.
                        // LDS executes a wave's instructions in order, so these reads see the writes above and the next
                        // half's writes land behind them; the compiler is kept from reordering by the clobbers.
                        asm volatile("" ::: "memory");
                        __builtin_amdgcn_sched_barrier(0);
                        // the 16 rows as a 16 x 32 A operand per k-group of 32 image columns: lane l -> row l&15,
                        // columns 32 kg + 8 (l>>4) + j — every lane carries data (no zero half as a 32-row shape would)
                        const float* ar = img + (lane & 15) * ZC_IS + 8 * (lane >> 4);
#pragma unroll
                        for (int kg = 0; kg < SYNTH_TILE / 32; ++kg) {
                            const float4 q0 = *reinterpret_cast<const float4*>(ar + 32 * kg),
                                         q1 = *reinterpret_cast<const float4*>(ar + 32 * kg + 4);
                            const float f[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                            const Frag za = M::from8(f);
#pragma unroll
                            for (int nt = 0; nt < NT16; ++nt) {
                                Frag db;
                                db.h = colfrag16(sd, Ks, 32 * kg, nt * 16, lane);
                                db.m = colfrag16(sd + plane, Ks, 32 * kg, nt * 16, lane);
                                db.l = colfrag16(sd + 2 * plane, Ks, 32 * kg, nt * 16, lane);
                                mma16_split(accv[0][grp >> 2][nt], za, db);
                            }
                            __builtin_amdgcn_sched_barrier(0);   // one k-group at a time: hoisted reads of later ones cost registers
                        }
                        asm volatile("" ::: "memory");
                    }
                }
            }
            if constexpr (RB == 2) {                              // the other block's accumulators become the current ones
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                    for (int nt = 0; nt < NT16; ++nt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float t = accv[0][hf][nt][r];
                            accv[0][hf][nt][r] = accv[1][hf][nt][r];
                            accv[1][hf][nt][r] = t;
                        }
            }
        }
    }
    // (after a whole number of slices accv[0] is block 0's again: two trades per slice, also for blocks beyond the batch)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {                             // partial sums of this workgroup: slab[blockIdx.x][row][atom < K]
        const int b0 = wrow0 + rb * 32;
        if (b0 < Bp) {
            float* dst = slab + (size_t)blockIdx.x * Bp * K;
            const int l16 = lane & 15, q4 = lane >> 4;            // C layout of the 16 x 16 tiles: rows 4 q4 + r, column l16
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int nt = 0; nt < NT16; ++nt)
                    if (nt * 16 + l16 < K) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            dst[(size_t)(b0 + 16 * hf + 4 * q4 + r) * K + nt * 16 + l16] = accv[rb][hf][nt][r];
                    }
        }
    }
    if (max_abs_delta != nullptr) {
        dmax = wave_max(dmax);
        if (lane == 0 && dmax > 0.0f) atomic_max_nonneg(max_abs_delta, dmax);
    }
}

// =========================================================================================================== //
// K7  Gram matrix D^T D (adil.py:523), K x K, fp32-grade on the bf16 matrix pipe.  The D tile of 32 pixels is staged
// exactly as in grad_v_f32_kernel (transposed, three bf16 planes, [atom][pixel]) — and serves as BOTH MFMA operands: the
// fragments of atom tile i (lane = atom, 8 consecutive pixels) against those of atom tile j.  8 waves share the AT x AT
// output tiles; partial sums per workgroup, reduced in a fixed order by grad_v_reduce_kernel (bitwise reproducible).
// Round 1-2 had a scalar-FMA kernel here: 258 us at K = 50, 3.2 ms at K = 100; this one reads D once (30 / 60 MB).
// =========================================================================================================== //
template <int AT>
__global__ __launch_bounds__(512) void gram_mfma_kernel(const float* __restrict__ d, float* __restrict__ partial, int P, int K,
                                                        int ntiles, int tiles_per_wg) {
    using M = Mma<float>;
    constexpr int TW = 32, KA = AT * 32, NT = 512, NW = 8;
    constexpr int GD = TW + DPAD, DPL = KA * GD, DBUF = 3 * DPL;
    constexpr int DPT = (TW * KA + NT - 1) / NT;
    constexpr int NOUT = AT * AT, MAXT = (NOUT + NW - 1) / NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sdt = reinterpret_cast<bf16_t*>(smem_raw);           // [2][3][KA][GD]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int t0 = blockIdx.x * tiles_per_wg;
    const int t1 = min(ntiles, t0 + tiles_per_wg);
    f32x16 acc[MAXT];
#pragma unroll
    for (int q = 0; q < MAXT; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;
    float dreg[DPT];
    auto load_d = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < DPT; ++e) {
            const int i = tid + e * NT;
            const int px = i / KA, a = i - px * KA;
            const int pix = tile * TW + (px < TW ? px : TW - 1);
            dreg[e] = d[(size_t)(pix < P ? pix : P - 1) * K + (a < K ? a : K - 1)];
        }
    };
    auto write_d = [&](bf16_t* dst, int tile) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < DPT; ++e) {
            const int i = tid + e * NT;
            const int px = i / KA, a = i - px * KA;
            const float keep = (a < K && tile * TW + px < P) ? 1.0f : 0.0f;     // atom / pixel tails: multiply, never a select
            if (px < TW) DImg<float>::put(dst, a * GD + px, DPL, dreg[e] * keep);
        }
    };
    if (t0 < t1) { load_d(t0); write_d(sdt, t0); }
    for (int tile = t0; tile < t1; ++tile) {
        const int buf = (tile - t0) & 1;
        if (tile + 1 < t1) load_d(tile + 1);
        lds_barrier();                                          // D[buf] visible; everyone is done reading D[buf^1]
        const bf16_t* sdb = sdt + buf * DBUF;
#pragma unroll
        for (int q = 0; q < MAXT; ++q) {
            const int o = w + q * NW;                             // output tile (ti, tj), wave-uniform
            if (o < NOUT) {
                const int ti = o / AT, tj = o - ti * AT;
#pragma unroll
                for (int g3 = 0; g3 < TW / 16; ++g3)
                    M::mma(acc[q], DImg<float>::load8(sdb + (ti * 32 + c) * GD + 16 * g3 + 8 * h, DPL),
                           DImg<float>::load8(sdb + (tj * 32 + c) * GD + 16 * g3 + 8 * h, DPL));
            }
        }
        if (tile + 1 < t1) write_d(sdt + (buf ^ 1) * DBUF, tile + 1);
    }
    float* dst = partial + (size_t)blockIdx.x * K * K;
#pragma unroll
    for (int q = 0; q < MAXT; ++q) {
        const int o = w + q * NW;
        if (o < NOUT) {
            const int ti = o / AT, tj = o - ti * AT;
            const int j = tj * 32 + c;
            if (j < K) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = ti * 32 + c_row(r, h);
                    if (i < K) dst[(size_t)i * K + j] = acc[q][r];
                }
            }
        }
    }
}

// =========================================================================================================== //
// K7  out (P x K) = D M^T with M (K x K): D_dagger^T = D (DtD)^-1 (adil.py:525), fp32-grade on the bf16 matrix pipe.
// M is staged once per workgroup (rows of M = output atoms, three bf16 planes, zero padded); the workgroup then walks
// 32-pixel blocks of D: the block (one contiguous run of 32*K floats) goes to LDS as planes [pixel][atom] with coalesced
// 16-byte loads (double buffered), wave t multiplies it with the rows of atom tile t of M and stores its 32 x 32 tile of
// the result with the lanes along the atoms.  Round 1-2 had a scalar-FMA kernel here (76 us at K = 50, ~370 us at K = 100).
// =========================================================================================================== //
template <int AT>
__global__ __launch_bounds__(AT * 64) void dict_rightmul_mfma_kernel(const float* __restrict__ d, const float* __restrict__ mat,
                                                                     float* __restrict__ out, int P, int K, int Kp, int nblocks) {
    using M = Mma<float>;
    using DI = DImg<float>;
    constexpr int NT = AT * 64, KA = AT * 32;
    const int Ks = Kp + DPAD;
    const int mplane = KA * Ks, dplane = 32 * Ks;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sm = reinterpret_cast<bf16_t*>(smem_raw);            // [3][KA][Ks]   M, row = output atom
    bf16_t* sdb = sm + 3 * mplane;                               // [2][3][32][Ks]  D block, row = pixel
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    for (int i = tid; i < KA * Kp; i += NT) {                     // M -> planes (zero rows / columns beyond K)
        const int r = i / Kp, k = i - r * Kp;
        const float ok = (r < K && k < K) ? 1.0f : 0.0f;
        DI::put(sm, r * Ks + k, mplane, mat[(size_t)(r < K ? r : K - 1) * K + (k < K ? k : K - 1)] * ok);
    }
    constexpr int DPT = (32 * KA + NT - 1) / NT;                  // elements of a 32 x Kp block per thread (Kp <= KA): 16
    float dreg[DPT];
    auto load_block = [&](int blk) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < DPT; ++e) {
            const int i = tid + e * NT;
            const int r = i / Kp, k = i - r * Kp;
            const int pix = blk * 32 + (r < 32 ? r : 31);
            dreg[e] = d[(size_t)(pix < P ? pix : P - 1) * K + (k < K ? k : K - 1)];
        }
    };
    auto write_block = [&](bf16_t* dst, int blk) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < DPT; ++e) {
            const int i = tid + e * NT;
            const int r = i / Kp, k = i - r * Kp;
            if (r < 32) DI::put(dst, r * Ks + k, dplane, dreg[e] * ((k < K && blk * 32 + r < P) ? 1.0f : 0.0f));
        }
    };
    const int NG = Kp >> 4;
    int blk = blockIdx.x;
    if (blk < nblocks) { load_block(blk); write_block(sdb, blk); }
    int buf = 0;
    for (; blk < nblocks; blk += gridDim.x, buf ^= 1) {
        const int nxt = blk + gridDim.x;
        if (nxt < nblocks) load_block(nxt);
        lds_barrier();                                          // M and block[buf] visible; block[buf^1] free
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const bf16_t* sblk = sdb + buf * 3 * dplane;
        for (int g = 0; g < NG; ++g)
            M::mma(acc, DI::load8(sblk + c * Ks + 16 * g + 8 * h, dplane), DI::load8(sm + (w * 32 + c) * Ks + 16 * g + 8 * h, mplane));
        const int atom = w * 32 + c;
        if (atom < K) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int pix = blk * 32 + c_row(r, h);
                if (pix < P) out[(size_t)pix * K + atom] = acc[r];
            }
        }
        if (nxt < nblocks) write_block(sdb + (buf ^ 1) * 3 * dplane, nxt);
    }
}

// codes transposed + converted to the MFMA element type: vpt[a][b] = vp[b][a]  (a < KA, b < Bp)
template <typename E>
__global__ __launch_bounds__(256) void transpose_codes_kernel(const float* __restrict__ vp, int Bp, int Kp, int KA,
                                                              E* __restrict__ vpt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= KA * Bp) return;
    const int a = i / Bp, b = i - a * Bp;
    const float v = (a < Kp) ? vp[(size_t)b * Kp + a] : 0.0f;
    if constexpr (sizeof(E) == 4) vpt[i] = v; else vpt[i] = f32_to_bf16(v);
}

// grad_vb[b][k] = sum over the workgroup slabs (slab_sum: fixed order, 32 loads in flight per lane).  One entry per lane.
// Used when the reduction cannot be left to the consumer (several row chunks share the slab area, or the caller asked
// for a dense grad_vb); adil_adamw_l1ball / adil_pack_codes run the same sum inside their own launch otherwise.
__global__ __launch_bounds__(64) void grad_v_reduce_kernel(const float* __restrict__ slab, int nslabs, int Bp, int KA,
                                                           int B, int K, float* __restrict__ grad_vb) {
    const int e = blockIdx.x * 64 + threadIdx.x;                 // entry of the [Bp][KA] slab matrix (KA = row stride = K)
    if (e >= Bp * KA) return;
    const int b = e / KA, k = e - b * KA;
    if (b < B && k < K) grad_vb[(size_t)b * K + k] = slab_sum(slab + e, nslabs, (size_t)Bp * KA);
}

// =========================================================================================================== //
// C ABI
// =========================================================================================================== //
static inline int num_cu() { return adil_num_cu(); }     // 256 on MI355X (from hipDeviceAttributeMultiprocessorCount)
static inline int imin(int a, int b) { return a < b ? a : b; }
static inline int half_cu() { return num_cu() / 2 > 0 ? num_cu() / 2 : 1; }    // two workgroups per range, one per CU

// Dynamic LDS above 48 KB has to be allowed per kernel function; asked of the runtime once per (device, function, size),
// not on every launch.
static int set_lds(const void* fn, size_t bytes) {
    if (bytes <= 48 * 1024) return 0;
    static std::mutex mu;
    static std::unordered_map<const void*, size_t> allowed[32];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return (int)hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(mu);
    auto it = allowed[dev].find(fn);
    if (it != allowed[dev].end() && it->second >= bytes) return 0;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
    allowed[dev][fn] = bytes;
    return 0;
}

// Every launch of this file: allow its LDS, launch, return the launch error.  The arguments convert to the kernel's
// parameters; its default arguments do not apply through the pointer, so all of them are passed.
template <typename... Params, typename... Args>
static int launch(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    int rc = set_lds((const void*)kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    ADIL_CHECK_LAUNCH();
    return 0;
}

// Runtime values as template arguments: f(std::true_type / std::false_type), f(TypeTag<stream type>), f(integral_constant AT)
template <typename F> static int with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

template <typename T> struct TypeTag { using type = T; };
template <typename F> static int with_dtype(int dtype, F&& f) {
    if (dtype == ADIL_F32) return f(TypeTag<float>{});
    if (dtype == ADIL_BF16) return f(TypeTag<bf16_t>{});
    return ADIL_EINVAL;
}

static inline int atom_tiles(int K) { return (K + 31) / 32; }
static inline int grad_at(int K) { const int a = atom_tiles(K); return a <= 2 ? a : 4; }       // instantiated: 1, 2, 4
template <typename F> static int with_atom_tiles(int K, F&& f) {
    const int at = grad_at(K);
    if (at == 1) return f(std::integral_constant<int, 1>{});
    if (at == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 4>{});
}

// Pixel tiles of width `tw`: [0, nfast) go through the FAST (vector-aligned) kernel when the caller's `vec` holds,
// [nfast, ntiles) through the element-wise one.
struct TileSplit {
    int ntiles, nfast;
    TileSplit(int P, int tw, bool vec) : ntiles((P + tw - 1) / tw), nfast(vec ? P / tw : 0) {}
    int nslow() const { return ntiles - nfast; }
};
// n tiles over at most `slots` workgroups: tpw tiles per workgroup, nwg workgroups (none for no tiles)
struct Spread {
    int tpw, nwg;
    Spread(int n, int slots) : tpw(n > 0 ? (n + slots - 1) / slots : 1), nwg(n > 0 ? (n + tpw - 1) / tpw : 0) {}
};
// k-split launches (two workgroups per tile range share out the atoms): 16 workgroups per 8 ranges
static inline int k_split_grid(int nranges) { return 16 * ((nranges + 7) / 8); }

// ---- K7 Gram ------------------------------------------------------------------------------------------------ //
extern "C" size_t adil_gram_workspace_bytes(int P, int K) { (void)P; return (size_t)num_cu() * K * K * sizeof(float); }

extern "C" int adil_gram(const float* d, int P, int K, float* gram, void* ws, size_t ws_bytes, void* stream) {
    ADIL_ENTER();
    if (!d || !gram || !ws || P <= 0 || K <= 0 || K > ADIL_MAX_ATOMS) return ADIL_EINVAL;
    if (ws_bytes < adil_gram_workspace_bytes(P, K)) return ADIL_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nt = (P + 31) / 32;
    const Spread r(nt, num_cu());
    const int rc = with_atom_tiles(K, [&](auto at) {
        constexpr int AT = decltype(at)::value;
        const size_t lds = 2 * 3 * (size_t)AT * 32 * (32 + DPAD) * sizeof(bf16_t);
        return launch(gram_mfma_kernel<AT>, dim3(r.nwg), dim3(512), lds, st, d, (float*)ws, P, K, nt, r.tpw);
    });
    if (rc) return rc;
    return launch(grad_v_reduce_kernel, dim3((K * K + 63) / 64), dim3(64), 0, st, (const float*)ws, r.nwg, K, K, K, K, gram);
}

// ---- K7 D M^T ----------------------------------------------------------------------------------------------- //
extern "C" int adil_dict_rightmul(const float* d, const float* mat, int P, int K, float* out, void* stream) {
    ADIL_ENTER();
    if (!d || !mat || !out || P <= 0 || K <= 0 || K > ADIL_MAX_ATOMS) return ADIL_EINVAL;
    const int Kp = round_up(K, 16), Ks = Kp + DPAD, nblocks = (P + 31) / 32;
    const int grid = nblocks < 4 * num_cu() ? nblocks : 4 * num_cu();
    return with_atom_tiles(K, [&](auto at) {
        constexpr int AT = decltype(at)::value;
        const size_t lds = (3 * (size_t)AT * 32 * Ks + 2 * 3 * (size_t)32 * Ks) * sizeof(bf16_t);
        return launch(dict_rightmul_mfma_kernel<AT>, dim3(grid), dim3(AT * 64), lds, (hipStream_t)stream, d, mat, out, P, K,
                      Kp, nblocks);
    });
}

extern "C" size_t adil_grad_workspace_bytes(int B, int P, int K) {
    (void)P;
    const size_t KA = grad_at(K) * 32, Bp = round_up(B, 32);
    const size_t vpt = KA * Bp * sizeof(float);                       // transposed codes (grad_d)
    const size_t rows = Bp < 512 ? Bp : 512;
    const size_t slab = (size_t)(2 * num_cu() + 2) * rows * KA * sizeof(float);   // grad_v partial sums per workgroup
    return ((vpt + 255) / 256) * 256 + slab;
}

// ---- synthesis ---------------------------------------------------------------------------------------------- //
// One tile range [tile0, tile0 + ntiles), a workgroup per tile.  STORE: x rows index[b] of the 8-bit store (xidx).
template <typename T, typename O, bool XACC, bool FAST, bool STORE>
static int launch_synth_range(const void* x, const float* d, const float* vp, void* out, int B, int P, int K,
                              float delta_clamp, int pixel_clamp, int tile0, int ntiles, OpScale sc, const int64_t* xidx,
                              hipStream_t st) {
    if (ntiles <= 0) return 0;
    const int Kp = round_up(K, 16);
    const size_t lds = (size_t)DImg<O>::PLANES * SYNTH_TILE * (Kp + DPAD) * sizeof(typename DImg<O>::Elem) +
                       (STORE ? 256 * sizeof(float) : 0);     // + the byte -> value table of an 8-bit store
    auto run = [&](auto kernel, int nthreads) {
        return launch(kernel, dim3(ntiles), dim3(nthreads), lds, st, (const T*)x, d, vp, (T*)out, B, P, K, Kp, delta_clamp,
                      pixel_clamp, tile0, sc, xidx);
    };
    if constexpr (FAST) {
        if (Kp > 64) {
            // all k-groups' code fragments hoisted (see synth_sweep_buf) — but fp32 operands take 12 registers per split
            // fragment and 8 do not fit: there 92 KB of D planes = one workgroup per CU, so 8 waves instead of 4
            if constexpr (sizeof(typename Mma<O>::Frag) <= 16)
                return run(synth_mfma_kernel<T, O, XACC, true, 8, 4, false, STORE>, 256);
            else
                return run(synth_mfma_kernel<T, O, XACC, true, 4, 8, false, STORE>, 512);
        }
    }
    return run(synth_mfma_kernel<T, O, XACC, FAST, 4, 4, false, STORE>, 256);
}

// full (interior, vector-aligned) tiles go through the FAST kernel, the ragged tail / unaligned rows through the
// element-wise one
template <typename T, typename O, bool XACC, bool STORE = false>
static int launch_synth_tiles(bool vec, const void* x, const float* d, const float* vp, void* out, int B, int P, int K,
                              float delta_clamp, int pixel_clamp, OpScale sc, const int64_t* xidx, hipStream_t st) {
    const TileSplit t(P, SYNTH_TILE, vec);
    int rc = launch_synth_range<T, O, XACC, true, STORE>(x, d, vp, out, B, P, K, delta_clamp, pixel_clamp, 0, t.nfast, sc,
                                                         xidx, st);
    if (rc) return rc;
    return launch_synth_range<T, O, XACC, false, STORE>(x, d, vp, out, B, P, K, delta_clamp, pixel_clamp, t.nfast, t.nslow(),
                                                        sc, xidx, st);
}

// (stream dtype, x rides in the accumulator) -> f(TypeTag<T>, bool_constant<XACC>)
template <typename F> static int with_synth_cfg(int dtype, bool xacc, F&& f) {
    return with_dtype(dtype, [&](auto t) { return with_bool(xacc, [&](auto xa) { return f(t, xa); }); });
}

// fp8 operands: codes |v| <= v_absmax -> |v sc.v| <= 384 < 448 (e4m3 max normal); dictionary |D| <= 1 (update_d clamps
// it, adil.py:33-35)
static OpScale fp8_scale(float v_absmax) {
    OpScale sc;
    sc.v = 384.0f / v_absmax;
    sc.d = 256.0f;
    sc.o = 1.0f / (sc.v * sc.d);
    return sc;
}

extern "C" int adil_synth_fp8(const void* x, const float* d, const float* vp, void* out, int B, int P, int K, int dtype,
                              float v_absmax, float delta_clamp, int pixel_clamp, void* stream) {
    ADIL_ENTER();
    if (!d || !vp || !out || B <= 0 || P <= 0 || K <= 0 || K > ADIL_MAX_ATOMS || !(v_absmax > 0.0f)) return ADIL_EINVAL;
    const OpScale sc = fp8_scale(v_absmax);
    const bool vec = (P % 4 == 0) && (((uintptr_t)out | (uintptr_t)x | (uintptr_t)d) % 16 == 0) && (P <= (1 << 23));
    const bool xacc = (x != nullptr) && (delta_clamp < 0.0f);    // x rides in the accumulator, pre-multiplied by vscale*dscale
    return with_synth_cfg(dtype, xacc, [&](auto t, auto xa) {
        return launch_synth_tiles<typename decltype(t)::type, fp8_t, decltype(xa)::value>(
            vec, x, d, vp, out, B, P, K, delta_clamp, pixel_clamp, sc, nullptr, (hipStream_t)stream);
    });
}

extern "C" int adil_synth_fp8_packed(const void* x, const void* d_fp8, const float* vp, void* out, int B, int P, int K, int dtype,
                                     float v_absmax, float delta_clamp, int pixel_clamp, void* stream) {
    ADIL_ENTER();
    if (!d_fp8 || !vp || !out || B <= 0 || P <= 0 || K <= 0 || K > ADIL_MAX_ATOMS || !(v_absmax > 0.0f)) return ADIL_EINVAL;
    // whole 128-pixel slices of 4-byte groups, 16-byte aligned streams: everything else goes through adil_synth_fp8
    if (P % SYNTH_TILE != 0 || K % 4 != 0 || P > (1 << 23) || (((uintptr_t)out | (uintptr_t)x) % 16) != 0 || ((uintptr_t)d_fp8 % 4) != 0)
        return ADIL_EINVAL;
    const OpScale sc = fp8_scale(v_absmax);
    const int Kp = round_up(K, 16);
    const size_t lds = (size_t)SYNTH_TILE * (Kp + DPAD);
    const bool xacc = (x != nullptr) && (delta_clamp < 0.0f);
    return with_synth_cfg(dtype, xacc, [&](auto t, auto xa) {
        using T = typename decltype(t)::type;
        constexpr bool XACC = decltype(xa)::value;
        auto run = [&](auto kernel) {
            return launch(kernel, dim3(P / SYNTH_TILE), dim3(256), lds, (hipStream_t)stream, (const T*)x, (const float*)d_fp8,
                          vp, (T*)out, B, P, K, Kp, delta_clamp, pixel_clamp, 0, sc, (const int64_t*)nullptr);
        };
        return Kp > 64 ? run(synth_mfma_kernel<T, fp8_t, XACC, true, 8, 4, true>)
                       : run(synth_mfma_kernel<T, fp8_t, XACC, true, 4, 4, true>);
    });
}

extern "C" int adil_synth(const void* x, const float* d, const float* vp, void* out, int B, int P, int K, int dtype,
                          float delta_clamp, int pixel_clamp, void* stream) {
    ADIL_ENTER();
    if (!d || !vp || !out || B <= 0 || P <= 0 || K <= 0 || K > ADIL_MAX_ATOMS) return ADIL_EINVAL;
    // FAST = vector-aligned rows, and a 32-row block addressable with 32-bit byte offsets (buffer instructions)
    const bool vec = (P % 4 == 0) && (((uintptr_t)out | (uintptr_t)x | (uintptr_t)d) % 16 == 0) && (P <= (1 << 23));
    const bool xacc = (x != nullptr) && (delta_clamp < 0.0f);
    return with_synth_cfg(dtype, xacc, [&](auto t, auto xa) {
        using T = typename decltype(t)::type;
        return launch_synth_tiles<T, T, decltype(xa)::value>(vec, x, d, vp, out, B, P, K, delta_clamp, pixel_clamp,
                                                              OpScale{1.0f, 1.0f, 1.0f}, nullptr, (hipStream_t)stream);
    });
}

extern "C" int adil_synth_store(const uint8_t* store, const int64_t* index, const float* d, const float* vp, void* out, int B,
                                int P, int K, int out_dtype, float delta_clamp, int pixel_clamp, void* stream) {
    ADIL_ENTER();
    if (!store || !index || !d || !vp || !out || B <= 0 || P <= 0 || (P & 7) || K <= 0 || K > ADIL_MAX_ATOMS) return ADIL_EINVAL;
    if ((uintptr_t)store & 3) return ADIL_EINVAL;
    // the same tile split as adil_synth, x read out of the 8-bit store (never through buffer instructions, so only out
    // and d decide which tiles are FAST)
    const bool vec = (((uintptr_t)out | (uintptr_t)d) % 16 == 0) && (P <= (1 << 23));
    const bool xacc = delta_clamp < 0.0f;                         // as adil_synth with x present
    return with_synth_cfg(out_dtype, xacc, [&](auto t, auto xa) {
        using T = typename decltype(t)::type;
        return launch_synth_tiles<T, T, decltype(xa)::value, true>(vec, store, d, vp, out, B, P, K, delta_clamp, pixel_clamp,
                                                                    OpScale{1.0f, 1.0f, 1.0f}, index, (hipStream_t)stream);
    });
}

// ---- grad ------------------------------------------------------------------------------------------------------ //
// adil_grad's operands.  The slabs (grad_v partial sums, one per workgroup) follow the transposed codes in the workspace.
template <typename T> struct Grad {
    using E = typename Mma<T>::Elem;
    const T* g;
    const float* d;
    float* grad_d;
    float* grad_vb;
    int B, Bp, P, K, accumulate_d;
    const E* vpt;         // vpt[a][b] = vp[b][a], KA x Bp (grad_d)
    float* slab;
    int* nslabs_out;      // non-null: the caller reduces the grad_v slabs itself (adil_adamw_l1ball / adil_pack_codes) when
                          // ONE row chunk covers the batch; receives the slab count, 0 = reduced here into grad_vb as usual
    hipStream_t st;
    // FAST tiles at all: rows of a multiple of `p_multiple` pixels (each route has its own) on a 16-byte aligned g
    bool vec(int p_multiple) const { return P % p_multiple == 0 && (uintptr_t)g % 16 == 0; }
};

// Row chunks of `chunk` rows, the last one ragged: run(r0, rows, rows_p, acc_d) launches one chunk's kernels; grad_d
// accumulates from the second chunk on.  The `nslabs` grad_v slabs a chunk leaves (0: grad_d only) then go to the
// caller (one chunk covers the batch) or are reduced here into the chunk's rows of grad_vb (slab rows are K wide).
template <typename T, typename F>
static int for_row_chunks(const Grad<T>& a, int chunk, int nslabs, F&& run) {
    for (int r0 = 0; r0 < a.Bp; r0 += chunk) {
        const int rows_p = imin(a.Bp - r0, chunk), rows = imin(a.B - r0, rows_p);
        int rc = run(r0, rows, rows_p, a.accumulate_d || r0 > 0);
        if (rc == 0 && nslabs > 0) {
            if (a.nslabs_out != nullptr && a.Bp <= chunk) *a.nslabs_out = nslabs;
            else rc = launch(grad_v_reduce_kernel, dim3((rows_p * a.K + 63) / 64), dim3(64), 0, a.st, (const float*)a.slab,
                             nslabs, rows_p, a.K, rows, a.K, a.grad_vb + (size_t)r0 * a.K);
        }
        if (rc) return rc;
    }
    return 0;
}

// rows per fused launch, bounded by LDS (one image per 32 rows + partials); the fused pass runs for K <= 64 only
template <typename T> struct FusedCfg { static constexpr int kMaxRows = sizeof(T) == 2 ? 512 : 256; };

// waves (= 32-row blocks) per grad_v workgroup, bounded by LDS: fp32 streams stage three planes of the D tile
template <typename T, int AT> struct GradVWaves { static constexpr int kMax = sizeof(T) == 2 ? 16 : (AT <= 2 ? 8 : 4); };

template <typename T, int AT>
static size_t grad_v_lds_bytes(int nwaves) {
    using E = typename Mma<T>::Elem;
    const size_t GS = GV_TW + Mma<T>::PAD, GD = GV_TW + DPAD;
    return 2 * (size_t)DImg<T>::PLANES * AT * 32 * GD * sizeof(bf16_t) + (size_t)nwaves * 32 * GS * sizeof(E);
}

// WV = false: grad_d alone, no D planes
template <typename T, int AT, int NW, int RB, bool WV = true>
static size_t grad_fused_lds_bytes() {
    using E = typename Mma<T>::Elem;
    const size_t GS = GV_TW + Mma<T>::PAD, GD = GV_TW + DPAD;
    return (WV ? 2 * (size_t)DImg<T>::PLANES * AT * 32 * GD * sizeof(bf16_t) : 0) + (size_t)NW * RB * 32 * GS * sizeof(E) +
           (size_t)NW * 16 * 64 * sizeof(float);
}

// One row chunk of grad_fused_mfma_kernel: the FAST tiles on ranges f, then the slow tail on ranges s, whose slabs follow
// the fast ones.  k_split > 0: two workgroups per range, [0, k_split) and [k_split, K) of the atoms.
template <typename T, int AT, int NW, int RB, bool WV = true>
static int launch_grad_fused_chunk(const Grad<T>& a, int r0, int rows, int rows_p, bool acc_d, const TileSplit& t,
                                   const Spread& f, const Spread& s, int k_split = 0) {
    auto run = [&](auto kernel, float* slab, int t0, int t1, const Spread& r) {
        if (r.nwg <= 0) return 0;
        return launch(kernel, dim3(k_split > 0 ? k_split_grid(r.nwg) : r.nwg), dim3(NW * 64),
                      grad_fused_lds_bytes<T, AT, NW, RB, WV>(), a.st, a.g + (size_t)r0 * a.P, WV ? a.d : nullptr, a.vpt + r0, a.Bp, a.grad_d, slab, rows, rows_p, a.P,
                      a.K, t0, t1, r.tpw, k_split, k_split > 0 ? r.nwg : 0);
    };
    return with_bool(acc_d, [&](auto acc) {
        constexpr bool ACC = decltype(acc)::value;
        int rc = run(grad_fused_mfma_kernel<T, AT, NW, RB, true, ACC, WV>, WV ? a.slab : nullptr, 0, t.nfast, f);
        if (rc) return rc;
        return run(grad_fused_mfma_kernel<T, AT, NW, RB, false, ACC, WV>, WV ? a.slab + (size_t)f.nwg * rows_p * a.K : nullptr,
                   t.nfast, t.ntiles, s);
    });
}

// ---- both outputs, 64 < K <= 128 on bf16 streams: two workgroups per tile range split the ATOMS ------------------- //
// (see grad_fused_mfma_kernel, k_split).  The K <= 64 instantiations (AT = 2 tiles, 8 waves x 2 row blocks = 512 rows) do
// the work; each half owns ceil(K/2) / floor(K/2) atoms.  One launch per 512-row chunk; later chunks accumulate into grad_d.
template <typename T>
static int launch_grad_fused_split(const Grad<T>& a) {
    const int kh = (a.K + 1) / 2;                                 // atoms of the first half; both halves <= 64
    const TileSplit t(a.P, GV_TW, a.vec(8));
    const Spread f(t.nfast, half_cu()), s(t.nslow(), half_cu());
    return for_row_chunks(a, 512, f.nwg + s.nwg, [&](int r0, int rows, int rows_p, bool acc_d) {
        if (rows_p > 256) return launch_grad_fused_chunk<T, 2, 8, 2>(a, r0, rows, rows_p, acc_d, t, f, s, kh);
        return launch_grad_fused_chunk<T, 2, 8, 1>(a, r0, rows, rows_p, acc_d, t, f, s, kh);
    });
}

// ---- both outputs, K <= 64: the generic fused pass, NW x RB row blocks from the chunk ------------------------------ //
template <typename T, int AT>
static int launch_grad_fused(const Grad<T>& a) {
    const TileSplit t(a.P, GV_TW, a.vec(8));
    const Spread f(t.nfast, num_cu()), s(t.nslow(), num_cu());
    return for_row_chunks(a, FusedCfg<T>::kMaxRows, f.nwg + s.nwg, [&](int r0, int rows, int rows_p, bool acc_d) {
        const int nblk = rows_p / 32;
        if constexpr (FusedCfg<T>::kMaxRows >= 512) {
            if (nblk > 8) return launch_grad_fused_chunk<T, AT, 8, 2>(a, r0, rows, rows_p, acc_d, t, f, s);
        }
        if (nblk > 4) return launch_grad_fused_chunk<T, AT, 8, 1>(a, r0, rows, rows_p, acc_d, t, f, s);
        return launch_grad_fused_chunk<T, AT, 4, 1>(a, r0, rows, rows_p, acc_d, t, f, s);
    });
}

// ---- fp32 streams, aligned rows, whole 32-pixel tiles: grad_fused_f32_kernel, every operand split once, 256 rows per
// launch.  WV = false: its grad_d half alone (K > 64, pre-split operands).
template <int AT, bool WV>
static int launch_grad_fused_f32(const Grad<float>& a) {
    constexpr int NW = 8, TW = 32;
    const int nt = a.P / TW;
    const Spread r(nt, num_cu());
    const size_t lds = ((WV ? 2 * 3 * (size_t)AT * 32 * (TW + DPAD) : 0) + 3 * (size_t)NW * 32 * (TW + DPAD)) * sizeof(bf16_t) +
                       (size_t)NW * 16 * 64 * sizeof(float);
    return for_row_chunks(a, NW * 32, WV ? r.nwg : 0, [&](int r0, int rows, int rows_p, bool acc_d) {
        return with_bool(acc_d, [&](auto acc) {
            return launch(grad_fused_f32_kernel<AT, NW, decltype(acc)::value, WV>, dim3(r.nwg), dim3(NW * 64), lds, a.st,
                          a.g + (size_t)r0 * a.P, WV ? a.d : nullptr, a.vpt + r0, a.Bp, a.grad_d, WV ? a.slab : nullptr, rows,
                          rows_p, a.P, a.K, nt, r.tpw);
        });
    });
}

// ---- grad_d alone through LDS (K > 64, bf16 streams): the grad_d half of the fused kernel, 512 rows per launch -------- //
template <typename T>
static int launch_grad_d_lds(const Grad<T>& a) {
    const TileSplit t(a.P, GV_TW, a.vec(8));
    const Spread f(t.nfast, num_cu()), s(t.nslow(), num_cu());
    return for_row_chunks(a, 512, 0, [&](int r0, int rows, int rows_p, bool acc_d) {
        if (rows_p > 256) return launch_grad_fused_chunk<T, 4, 8, 2, false>(a, r0, rows, rows_p, acc_d, t, f, s);
        return launch_grad_fused_chunk<T, 4, 8, 1, false>(a, r0, rows, rows_p, acc_d, t, f, s);
    });
}

// ---- grad_d alone, direct loads: grad_d_mfma_kernel, all rows per launch ------------------------------------------- //
template <typename T, int AT>
static int launch_grad_d(const Grad<T>& a) {
    constexpr int PXT = AT == 1 ? 4 : 2;                          // 32-pixel blocks per tile
    const TileSplit t(a.P, PXT * 32, a.vec(4));
    auto run = [&](auto kernel, int t0, int t1) {
        if (t1 <= t0) return 0;
        return launch(kernel, dim3((t1 - t0 + 3) / 4), dim3(256), 0, a.st, a.g, a.vpt, a.Bp, a.grad_d, a.B, a.Bp, a.P, a.K,
                      a.accumulate_d, t0, t1);
    };
    int rc = run(grad_d_mfma_kernel<T, PXT, AT, true>, 0, t.nfast);
    if (rc) return rc;
    return run(grad_d_mfma_kernel<T, PXT, AT, false>, t.nfast, t.ntiles);
}

// ---- grad_v alone, fp32 streams, aligned rows, whole 32-pixel tiles: grad_v_f32_kernel (planes split once), 512 rows per
// launch.  K > 64 (AT = 4): the AT = 2 shape with the atoms split over workgroup pairs — D read once, ONE slab per range,
// so a 512-row batch needs neither a second launch nor a reduce launch.
template <int AT>
static int launch_grad_v_f32(const Grad<float>& a) {
    constexpr int VAT = AT == 4 ? 2 : AT, TW = 32;
    const int nt = a.P / TW, k_split = AT == 4 ? (a.K + 1) / 2 : 0;
    const Spread r(nt, AT == 4 ? half_cu() : num_cu());
    return for_row_chunks(a, 512, r.nwg, [&](int r0, int rows, int rows_p, bool) {
        auto run = [&](auto kernel, int nw) {
            const size_t lds = (2 * 3 * (size_t)VAT * 32 * (TW + DPAD) + 3 * (size_t)nw * 32 * (TW + DPAD)) * sizeof(bf16_t);
            return launch(kernel, dim3(k_split > 0 ? k_split_grid(r.nwg) : r.nwg), dim3(nw * 64), lds, a.st,
                          a.g + (size_t)r0 * a.P, a.d, a.slab, rows, rows_p, a.P, a.K, nt, r.tpw, k_split,
                          k_split > 0 ? r.nwg : 0);
        };
        if (rows_p > 256) return run(grad_v_f32_kernel<VAT, 16>, 16);
        if (rows_p > 128) return run(grad_v_f32_kernel<VAT, 8>, 8);
        return run(grad_v_f32_kernel<VAT, 4>, 4);
    });
}

// ---- grad_v alone: grad_v_mfma_kernel, a wave per 32 rows of the chunk ------------------------------------------- //
template <typename T, int AT, int NW>
static int launch_grad_v_chunk(const Grad<T>& a, int r0, int rows, int rows_p, const TileSplit& t, const Spread& f,
                               const Spread& s) {
    auto run = [&](auto kernel, float* slab, int t0, int t1, const Spread& r) {
        if (r.nwg <= 0) return 0;
        return launch(kernel, dim3(r.nwg), dim3(NW * 64), grad_v_lds_bytes<T, AT>(NW), a.st, a.g + (size_t)r0 * a.P, a.d, slab,
                      rows, rows_p, a.P, a.K, t0, t1, r.tpw);
    };
    int rc = run(grad_v_mfma_kernel<T, AT, NW, true>, a.slab, 0, t.nfast, f);
    if (rc) return rc;
    return run(grad_v_mfma_kernel<T, AT, NW, false>, a.slab + (size_t)f.nwg * rows_p * a.K, t.nfast, t.ntiles, s);
}

template <typename T, int AT>
static int launch_grad_v(const Grad<T>& a) {
    constexpr int kMax = GradVWaves<T, AT>::kMax;
    const TileSplit t(a.P, GV_TW, a.vec(8));
    const Spread f(t.nfast, num_cu()), s(t.nslow(), num_cu());
    return for_row_chunks(a, kMax * 32, f.nwg + s.nwg, [&](int r0, int rows, int rows_p, bool) {
        const int nwaves = rows_p / 32;
        if constexpr (kMax >= 16) {
            if (nwaves > 8) return launch_grad_v_chunk<T, AT, 16>(a, r0, rows, rows_p, t, f, s);
        }
        if constexpr (kMax >= 8) {
            if (nwaves > 4) return launch_grad_v_chunk<T, AT, 8>(a, r0, rows, rows_p, t, f, s);
        }
        return launch_grad_v_chunk<T, AT, 4>(a, r0, rows, rows_p, t, f, s);
    });
}

// adil_grad's dispatch, in the order of the route table (ROUTES in tests/test_gpu_routes.py).
//
// A learning step wants both outputs from ONE pass over g while the batch fits four fused launches; every row chunk after
// the first ACCUMULATES into grad_d (the ACC variant: old tile values requested before the next tile's loads so that
// waiting for them does not drain the prefetch).  Measured, fused chunks vs the two single-output kernels: bf16 1024 rows
// K=50 (2 chunks) 128 vs 198 us; fp32 512 rows K=50 (2 chunks) 233 vs 242 us; bf16 2048 rows K=50 (4 chunks) 248 vs
// 360 us.  For K > 64 a fused launch holds 256 rows only (its grad_v accumulators), and the two single-output kernels,
// grad_d through LDS in 512-row launches, beat it from the second chunk on (512 rows 102 vs 135 us, 768 rows 194 vs 214,
// 1024 rows 253 vs 292); the atom-split pass beats both.
template <typename T, int AT>
static int launch_grad(const Grad<T>& a) {
    const bool both = a.grad_d != nullptr && a.grad_vb != nullptr;
    if constexpr (AT == 4 && sizeof(T) == 2) {
        // both outputs, bf16, K > 64, Bp <= 2048: the atom-split pass
        if (both && a.Bp <= 4 * 512) return launch_grad_fused_split(a);
    }
    if constexpr (AT <= 2) {
        if (both && a.Bp <= 4 * FusedCfg<T>::kMaxRows) {
            if constexpr (sizeof(T) == 4) {
                // both outputs, K <= 64, fp32, P % 32 == 0, g aligned: grad_fused_f32_kernel in 256-row chunks
                if (a.vec(32)) return launch_grad_fused_f32<AT, true>(a);
            }
            // both outputs, K <= 64: generic grad_fused_mfma_kernel, fast and slow ranges
            return launch_grad_fused<T, AT>(a);
        }
    }
    // otherwise grad_d and grad_v separately
    if (a.grad_d != nullptr) {
        int rc;
        if constexpr (AT == 4 && sizeof(T) == 2) {
            rc = launch_grad_d_lds(a);                                // grad_d, bf16, K > 64: through LDS, 512-row chunks
        } else if constexpr (AT == 4) {
            if (a.vec(32)) rc = launch_grad_fused_f32<4, false>(a);   // grad_d, fp32, K > 64, P % 32 == 0: 256-row chunks
            else rc = launch_grad_d<T, AT>(a);                        // grad_d, everything else: grad_d_mfma_kernel
        } else {
            rc = launch_grad_d<T, AT>(a);                             // grad_d, everything else: grad_d_mfma_kernel
        }
        if (rc) return rc;
    }
    if (a.grad_vb == nullptr) return 0;
    if constexpr (sizeof(T) == 4) {
        if (a.vec(32)) return launch_grad_v_f32<AT>(a);              // grad_v, fp32, P % 32 == 0: grad_v_f32_kernel
    }
    return launch_grad_v<T, AT>(a);                                  // grad_v, everything else: grad_v_mfma_kernel chunks
}

extern "C" int adil_grad_code_rows(int K) { return (K > 0 && K <= ADIL_MAX_ATOMS) ? grad_at(K) * 32 : 0; }

extern "C" size_t adil_grad_slab_offset(int B, int P, int K) {
    (void)P;
    return (((size_t)grad_at(K) * 32 * round_up(B, 32) * sizeof(float) + 255) / 256) * 256;
}

extern "C" int adil_grad(const void* g, const float* d, const float* vp, const void* vpt, float* grad_d, float* grad_vb,
                         int B, int P, int K, int dtype, int accumulate_d, void* ws, size_t ws_bytes, int* nslabs_out,
                         void* stream) {
    ADIL_ENTER();
    if (nslabs_out != nullptr) *nslabs_out = 0;
    if (!g || B <= 0 || P <= 0 || K <= 0 || K > ADIL_MAX_ATOMS) return ADIL_EINVAL;
    if (grad_d == nullptr && grad_vb == nullptr) return ADIL_EINVAL;
    if (grad_d != nullptr && !vp) return ADIL_EINVAL;
    if (grad_vb != nullptr && !d) return ADIL_EINVAL;
    if (vpt != nullptr && ((uintptr_t)vpt & 15)) return ADIL_EINVAL;
    if (!ws || ws_bytes < adil_grad_workspace_bytes(B, P, K)) return ADIL_EWORKSPACE;
    return with_dtype(dtype, [&](auto t) {
        return with_atom_tiles(K, [&](auto at) {
            using T = typename decltype(t)::type;
            using E = typename Mma<T>::Elem;
            constexpr int AT = decltype(at)::value;
            const int Bp = round_up(B, 32);
            float* slab = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(ws) + adil_grad_slab_offset(B, P, K));
            Grad<T> a{(const T*)g, d, grad_d, grad_vb, B, Bp, P, K, accumulate_d, reinterpret_cast<const E*>(vpt), slab,
                      grad_vb != nullptr ? nslabs_out : nullptr, (hipStream_t)stream};
            if (grad_d != nullptr && vpt == nullptr) {                // the codes transposed here (one small launch)
                E* vt = reinterpret_cast<E*>(ws);
                int rc = launch(transpose_codes_kernel<E>, dim3((AT * 32 * Bp + 255) / 256), dim3(256), 0, a.st, vp, Bp,
                                round_up(K, 16), AT * 32, vt);
                if (rc) return rc;
                a.vpt = vt;
            }
            return launch_grad<T, AT>(a);
        });
    });
}

// ---- K8: z-step ---------------------------------------------------------------------------------------------------- //
template <bool FAST>
static int launch_zstep_range(float* z, float* m, float* sq, const float* d, const float* vp, int B, int P, int K,
                              AdamWHyper hy, float lo, float hi, float* max_abs_delta, int tile0, int ntiles,
                              const float* skip_if_below, float skip_threshold, float* clear, const float* dyn,
                              hipStream_t st) {
    if (ntiles <= 0) return 0;
    const int Kp = round_up(K, 16);
    const size_t lds = (size_t)DImg<float>::PLANES * SYNTH_TILE * (Kp + DPAD) * sizeof(bf16_t);
    auto run = [&](auto kernel, int nthreads) {
        return launch(kernel, dim3(ntiles), dim3(nthreads), lds, st, z, m, sq, d, vp, B, P, K, Kp, hy, lo, hi, max_abs_delta,
                      tile0, skip_if_below, skip_threshold, clear, dyn);
    };
    if constexpr (FAST) {
        // 92 KB of D_dagger planes = one workgroup per CU: 8 waves instead of 4 (as synth)
        if (Kp > 64) return run(zstep_mfma_kernel<true, 8>, 512);
    }
    return run(zstep_mfma_kernel<FAST, 4>, 256);
}

// ---- K8 + K6: z-step that also leaves the next iteration's codes as slabs (zstep_codes_kernel) ---------------------- //
// Shapes the fused kernel takes: whole 128-pixel slices, 16-byte aligned rows addressable with 32-bit offsets, and an
// atom count whose D_dagger planes leave room for the eight 16 x 128 fp32 images in LDS (Kp <= 112).
static inline bool zstep_codes_shape_ok(int B, int P, int K) {
    return B > 0 && K > 0 && round_up(K, 16) <= 112 && P > 0 && P % SYNTH_TILE == 0 && P <= (1 << 23);
}
// rows one workgroup owns: 8 waves x RB blocks of 32 (RB = 2 while the accumulators of two blocks fit: K <= 64 and a batch
// that fills the second block); the row ranges beyond that go to blockIdx.y
static inline int zstep_codes_row_blocks(int B, int K) { return (atom_tiles(K) <= 2 && round_up(B, 32) > 256) ? 2 : 1; }
// One workgroup per CU: the pixel slices are cut into as many ranges as there are CUs PER ROW RANGE, so that the whole grid
// (ranges x row ranges) is resident at once — and a batch with ny row ranges leaves ny times fewer slabs (one per pixel
// range, all rows): at 512 x 100 atoms 118 ranges x 2 instead of 236 x 2 workgroups in two rounds, 24 MB of slabs instead of 48.
static inline void zstep_codes_grid(int B, int P, int K, int* nslices, int* spw, int* nwg, int* ny) {
    const int rows_per_wg = 8 * zstep_codes_row_blocks(B, K) * 32;
    *ny = (round_up(B, 32) + rows_per_wg - 1) / rows_per_wg;
    const int ranges = num_cu() / *ny > 0 ? num_cu() / *ny : 1;
    *nslices = P / SYNTH_TILE;
    *spw = (*nslices + ranges - 1) / ranges;
    *nwg = (*nslices + *spw - 1) / *spw;
}

extern "C" size_t adil_zstep_codes_slab_bytes(int B, int P, int K) {
    if (!zstep_codes_shape_ok(B, P, K)) return 0;
    int nslices, spw, nwg, ny;
    zstep_codes_grid(B, P, K, &nslices, &spw, &nwg, &ny);
    return (size_t)nwg * round_up(B, 32) * K * sizeof(float);
}

extern "C" int adil_zstep_codes(float* z, float* m, float* s, const float* dpinv_t, const float* gvp, int B, int P, int K,
                                float decay, float b1, float b2, float eps, float step_size, float bc2_sqrt, float lo, float hi,
                                float* max_abs_delta, const float* skip_if_below, float skip_threshold, float* clear,
                                const float* dyn_scalars, float* code_slabs, size_t code_slab_bytes, int* nslabs_out,
                                void* stream) {
    ADIL_ENTER();
    if (!z || !m || !s || !dpinv_t || !gvp || !code_slabs || !nslabs_out || B <= 0 || P <= 0 || K <= 0 || K > ADIL_MAX_ATOMS)
        return ADIL_EINVAL;
    *nslabs_out = 0;
    if (!zstep_codes_shape_ok(B, P, K)) return ADIL_EINVAL;
    if ((((uintptr_t)z | (uintptr_t)m | (uintptr_t)s | (uintptr_t)dpinv_t | (uintptr_t)code_slabs) % 16) != 0) return ADIL_EINVAL;
    if (code_slab_bytes < adil_zstep_codes_slab_bytes(B, P, K)) return ADIL_EWORKSPACE;
    const AdamWHyper hy{decay, b1, b2, eps, step_size, bc2_sqrt};
    const int Kp = round_up(K, 16), Bp = round_up(B, 32);
    int nslices, spw, nwg, ny;
    zstep_codes_grid(B, P, K, &nslices, &spw, &nwg, &ny);
    // accumulators per wave: RB blocks x AT atom tiles <= 4 (64 registers).  One block per wave when the batch leaves the
    // second one empty anyway.
    const bool two_blocks = zstep_codes_row_blocks(B, K) == 2;
    const int rc = with_atom_tiles(K, [&](auto at) {
        constexpr int AT = decltype(at)::value;
        const size_t lds = (size_t)3 * SYNTH_TILE * ZCodes<AT>::KS * sizeof(bf16_t) + (size_t)8 * 16 * ZC_IS * sizeof(float);
        auto run = [&](auto kernel) {
            return launch(kernel, dim3(nwg, ny), dim3(512), lds, (hipStream_t)stream, z, m, s, dpinv_t, gvp, code_slabs, B, Bp,
                          P, K, Kp, hy, lo, hi, max_abs_delta, nslices, spw, skip_if_below, skip_threshold, clear, dyn_scalars);
        };
        if constexpr (AT <= 2) {
            if (two_blocks) return run(zstep_codes_kernel<AT, 2>);
        }
        return run(zstep_codes_kernel<AT, 1>);
    });
    if (rc) return rc;
    *nslabs_out = nwg;
    return 0;
}

extern "C" int adil_zstep(float* z, float* m, float* s, const float* dpinv_t, const float* gvp, int B, int P, int K,
                          float decay, float b1, float b2, float eps, float step_size, float bc2_sqrt, float lo, float hi,
                          float* max_abs_delta, const float* skip_if_below, float skip_threshold, float* clear,
                          const float* dyn_scalars, void* stream) {
    ADIL_ENTER();
    if (!z || !m || !s || !dpinv_t || !gvp || B <= 0 || P <= 0 || K <= 0 || K > ADIL_MAX_ATOMS) return ADIL_EINVAL;
    const AdamWHyper hy{decay, b1, b2, eps, step_size, bc2_sqrt};
    const bool vec = (P % 4 == 0) && ((((uintptr_t)z | (uintptr_t)m | (uintptr_t)s | (uintptr_t)dpinv_t) % 16) == 0) &&
                     (P <= (1 << 23));                           // 32-row blocks addressable with 32-bit byte offsets
    const TileSplit t(P, SYNTH_TILE, vec);
    // `clear` is written by the first launch only (tile0 == 0 exists in exactly one of the two ranges)
    int rc = launch_zstep_range<true>(z, m, s, dpinv_t, gvp, B, P, K, hy, lo, hi, max_abs_delta, 0, t.nfast, skip_if_below,
                                      skip_threshold, t.nfast > 0 ? clear : nullptr, dyn_scalars, (hipStream_t)stream);
    if (rc) return rc;
    return launch_zstep_range<false>(z, m, s, dpinv_t, gvp, B, P, K, hy, lo, hi, max_abs_delta, t.nfast, t.nslow(),
                                     skip_if_below, skip_threshold, t.nfast > 0 ? nullptr : clear, dyn_scalars,
                                     (hipStream_t)stream);
}
