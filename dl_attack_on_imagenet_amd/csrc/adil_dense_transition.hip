// The transitions of the frozen DenseNet-121 — BatchNorm + ReLU, 1x1 convolution, AvgPool2d(2, 2) — with the pooling moved
// IN FRONT of the convolution (the two commute: both are linear and the 1x1 convolution is per pixel), forward and input
// gradient: adil_dense_transition_fwd / adil_dense_transition_bwd (include/adil_hip.h).  The GEMM runs on a quarter of the
// pixels and the full-resolution convolution output never exists.  bf16 channels_last storage, bf16 MFMA with fp32
// accumulation, one rounding to bf16 (RNE), no atomics, 64-bit element offsets.  Siblings of d1_kernel
// (adil_dense1x1.hip: same tiling, same MFMA roles, same tails, same XCD order), which stays as it is.
//
// Both directions are the row-major GEMM  OUT[M][O] = A'[M][R] . B[O][R]^T  with M = B H/2 W/2 POOLED pixels.  Pooled
// pixel mo = (b Ho + oh) Wo + ow owns the input pixels p00 = 2 (mo / Wo) W + 2 (mo % Wo), p00 + 1, p00 + W, p00 + W + 1
// (b H W + 2 oh W = 2 W (b Ho + oh): the image index needs no division of its own).
//   forward    A' = a = bf16(0.25 (((p00 + p01) + p10) + p11)), p = max(pre, 0) in fp32, pre = d1_pre's two roundings,
//              formed on the way from registers to LDS: the four input rows of a pooled pixel are gathered into registers
//              together (16 x 16 bytes in flight per thread, one chunk ahead of the MFMAs);  R = K, B = w [N][K], O = N;
//              the epilogue is the rounding alone
//   gradient   A' = g as stored, rows at a pitch of ldg;  R = N, B = wt [K][N], O = K;  epilogue: v = bf16((t pscale[k])
//              0.25) goes through LDS ONCE per pooled pixel, and on the way out each of the four input pixels keeps v
//              where its own pre > 0 and writes +0 elsewhere.  xin is fetched there, in the 16-byte chunks of the stores
//              (nothing of it is held under the reduction loop), and pre is recomputed by the forward's two operations.
//   Workgroup = 4 waves = 128 pooled pixels x BO output channels, BO = 32 CT, CT = 1 .. 5 picked as in d1_dispatch.
//   Tails as in d1_kernel: a 16-byte chunk past R and a B row past O are read at a clamped in-range address and replaced
//   by zeros on BOTH operands; a pooled row past M reads the window of row M - 1 and is not stored; a table entry past its
//   extent is read at a clamped index.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adil_common.h"
#include "adil_hip.h"
#include "adil_mfma.h"

namespace {

#define TR_BM 128
#define TR_BK 64
#define TR_LS (TR_BK + 8)              // LDS row stride (elements): 144 B = 9 x 16 B
#define TR_MAXC 2048

// d1_pre (adil_dense1x1.hip): product and sum each rounded to fp32, never one fma
__device__ __forceinline__ float tr_pre(float x, float ps, float pb) {
#pragma clang fp contract(off)
    const float p = x * ps;
    return p + pb;
}

// d1_kernel's order: the OT channel tiles of one pixel tile go to ONE XCD
__device__ __forceinline__ void tr_tile(int MT, int OT, int& mt, int& ot) {
    const int id = blockIdx.x, full = (MT >> 3) * 8 * OT;
    if (id < full) {
        const int xcd = id & 7, j = id >> 3;
        ot = j % OT;
        mt = (j / OT) * 8 + xcd;
    } else {
        const int r = id - full;
        ot = r % OT;
        mt = (MT >> 3) * 8 + r / OT;
    }
}

// first input pixel of the window of pooled pixel mo
__device__ __forceinline__ size_t tr_p00(int mo, int Wo, int W) {
    const int r = mo / Wo, ow = mo - r * Wo;
    return (size_t)2 * (size_t)r * (size_t)W + (size_t)(2 * ow);
}

// accumulators -> bf16 -> this wave's transposed buffer: lane = pixel c, quad q of tile ct = channels 32ct + 8q + 4h .. +3
template <int CT, bool SCALED>
__device__ __forceinline__ void tr_stage(const f32x16 (&acc)[CT], bf16_t* so, const float* otab, int c, int h) {
    constexpr int OS = 32 * CT + 8;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int co = 32 * ct + 8 * q + 4 * h;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = acc[ct][4 * q + e];
                if (SCALED) v[e] = (v[e] * otab[co + e]) * 0.25f;
            }
            u32x2 t;
            t[0] = pack2_bf16(v[0], v[1]);
            t[1] = pack2_bf16(v[2], v[3]);
            *reinterpret_cast<u32x2*>(so + c * OS + co) = t;
        }
    }
}

template <int CT>
__global__ __launch_bounds__(256) void tr_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ pscale,
                                                     const float* __restrict__ pshift, const bf16_t* __restrict__ bm,
                                                     bf16_t* __restrict__ out, int M, int R, int O, int Wo, int W, int MT,
                                                     int OT, int tab_off) {
    constexpr int BO = 32 * CT;
    constexpr int ACH = TR_BM * TR_BK / 8 / 256;         // 16-byte chunks of the A tile per thread (4), each from 4 pixels
    constexpr int OS = BO + 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sa = reinterpret_cast<bf16_t*>(smem_raw);    // [128][TR_LS]
    bf16_t* sb = sa + TR_BM * TR_LS;                     // [BO][TR_LS]
    float* rtab = reinterpret_cast<float*>(smem_raw + tab_off);          // pscale | pshift, zeros behind R
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    int mt, ot;
    tr_tile(MT, OT, mt, ot);
    const int m0 = mt * TR_BM, o0 = ot * BO;
    const int nk = (R + TR_BK - 1) / TR_BK, RP = nk * TR_BK;
    for (int i = tid; i < RP; i += 256) {
        const bool ok = i < R;
        const int ic = ok ? i : 0;
        const float v0 = pscale[ic], v1 = pshift[ic];
        rtab[i] = ok ? v0 : 0.0f;
        rtab[RP + i] = ok ? v1 : 0.0f;
    }
    __syncthreads();

    const size_t d01 = (size_t)R, d10 = (size_t)W * (size_t)R;
    size_t arow[ACH];
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
        const int row = (tid + 256 * i) >> 3;
        arow[i] = tr_p00(m0 + row < M ? m0 + row : M - 1, Wo, W) * (size_t)R;
    }
    u32x4 ar[ACH][4], br[CT];
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    auto load_tiles = [&](int kc) {
        const int col = kc * TR_BK + (tid & 7) * 8;
        const bool cok = col < R;
        const int colc = cok ? col : 0;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const bf16_t* p = x + arow[i] + colc;
            ar[i][0] = *reinterpret_cast<const u32x4*>(p);
            ar[i][1] = *reinterpret_cast<const u32x4*>(p + d01);
            ar[i][2] = *reinterpret_cast<const u32x4*>(p + d10);
            ar[i][3] = *reinterpret_cast<const u32x4*>(p + d10 + d01);
            if (!cok) {
#pragma unroll
                for (int j = 0; j < 4; ++j) ar[i][j] = zero4;
            }
        }
#pragma unroll
        for (int i = 0; i < CT; ++i) {
            const int n = o0 + ((tid + 256 * i) >> 3);
            const bool ok = cok && n < O;
            br[i] = *reinterpret_cast<const u32x4*>(bm + (ok ? (size_t)n * (size_t)R + colc : (size_t)0));
            if (!ok) br[i] = zero4;
        }
    };
    auto store_tiles = [&](int kc) {
        const int ch = tid & 7;
        const float* t0 = rtab + kc * TR_BK + ch * 8;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int row = (tid + 256 * i) >> 3;
            float s[8];
            // a zero-filled chunk past R meets zero table entries: pre = 0, p = +0, a = +0
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v[8];
                unpack8(ar[i][j], v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float pre = tr_pre(v[e], t0[e], t0[RP + e]);
                    const float p = pre > 0.0f ? pre : 0.0f;             // <= 0 (and -0.0, and NaN) -> +0
                    s[e] = j == 0 ? p : s[e] + p;                        // ((p00 + p01) + p10) + p11
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] *= 0.25f;
            *reinterpret_cast<u32x4*>(sa + row * TR_LS + ch * 8) = pack8(s);
        }
#pragma unroll
        for (int i = 0; i < CT; ++i) {
            const int row = (tid + 256 * i) >> 3;
            *reinterpret_cast<u32x4*>(sb + row * TR_LS + ch * 8) = br[i];
        }
    };

    load_tiles(0);
    f32x16 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.0f;
    for (int it = 0; it < nk; ++it) {
        store_tiles(it);
        if (it + 1 < nk) load_tiles(it + 1);
        lds_barrier();
        const bf16_t* bx = sa + (w * 32 + c) * TR_LS + 8 * h;
        const bf16_t* bw = sb + c * TR_LS + 8 * h;
        const int left = R - it * TR_BK;
        const int steps = left >= TR_BK ? TR_BK / 16 : (left + 15) / 16;
        for (int ks = 0; ks < steps; ++ks) {
            const bf16x8 b = lds8(bx + 16 * ks);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) mma16(acc[ct], lds8(bw + ct * 32 * TR_LS + 16 * ks), b);
        }
        lds_barrier();
    }
    bf16_t* so = reinterpret_cast<bf16_t*>(smem_raw) + w * 32 * OS;     // the tile buffers are idle now
    tr_stage<CT, false>(acc, so, nullptr, c, h);
    constexpr int CPP = BO / 8;                          // 16-byte chunks per pixel
#pragma unroll
    for (int i = 0; i < 32 * CPP / 64; ++i) {
        const int id = lane + 64 * i, px = id / CPP, ch = id - px * CPP;
        const u32x4 t = *reinterpret_cast<const u32x4*>(so + px * OS + ch * 8);
        const int mm = m0 + w * 32 + px, n = o0 + ch * 8;
        if (mm < M && n < O) *reinterpret_cast<u32x4*>(out + (size_t)mm * (size_t)O + n) = t;
    }
}

template <int CT>
__global__ __launch_bounds__(256) void tr_bwd_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ bm,
                                                     const bf16_t* __restrict__ xin, const float* __restrict__ pscale,
                                                     const float* __restrict__ pshift, bf16_t* __restrict__ out, int M, int R,
                                                     int O, int Wo, int W, int MT, int OT, int ldg) {
    constexpr int BO = 32 * CT;
    constexpr int ACH = TR_BM * TR_BK / 8 / 256;
    constexpr int OS = BO + 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sa = reinterpret_cast<bf16_t*>(smem_raw);    // [128][TR_LS]
    bf16_t* sb = sa + TR_BM * TR_LS;                     // [BO][TR_LS]
    __shared__ __attribute__((aligned(16))) float otab[2 * BO];          // pscale | pshift of this channel tile
    __shared__ int swin[TR_BM];                          // first input pixel of each pooled row's window (< 2^31)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    int mt, ot;
    tr_tile(MT, OT, mt, ot);
    const int m0 = mt * TR_BM, o0 = ot * BO;
    const int nk = (R + TR_BK - 1) / TR_BK;
    if (tid < BO) {
        const int n = o0 + tid < O ? o0 + tid : O - 1;
        otab[tid] = pscale[n];
        otab[BO + tid] = pshift[n];
    }
    if (tid < TR_BM) swin[tid] = (int)tr_p00(m0 + tid < M ? m0 + tid : M - 1, Wo, W);
    __syncthreads();

    size_t arow[ACH];
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
        const int row = (tid + 256 * i) >> 3;
        arow[i] = (size_t)((m0 + row < M) ? m0 + row : M - 1) * (size_t)ldg;
    }
    u32x4 ar[ACH], br[CT];
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    auto load_tiles = [&](int kc) {
        const int col = kc * TR_BK + (tid & 7) * 8;
        const bool cok = col < R;
        const int colc = cok ? col : 0;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            ar[i] = *reinterpret_cast<const u32x4*>(g + arow[i] + colc);
            if (!cok) ar[i] = zero4;
        }
#pragma unroll
        for (int i = 0; i < CT; ++i) {
            const int n = o0 + ((tid + 256 * i) >> 3);
            const bool ok = cok && n < O;
            br[i] = *reinterpret_cast<const u32x4*>(bm + (ok ? (size_t)n * (size_t)R + colc : (size_t)0));
            if (!ok) br[i] = zero4;
        }
    };
    auto store_tiles = [&]() {
        const int ch = tid & 7;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int row = (tid + 256 * i) >> 3;
            *reinterpret_cast<u32x4*>(sa + row * TR_LS + ch * 8) = ar[i];
        }
#pragma unroll
        for (int i = 0; i < CT; ++i) {
            const int row = (tid + 256 * i) >> 3;
            *reinterpret_cast<u32x4*>(sb + row * TR_LS + ch * 8) = br[i];
        }
    };

    load_tiles(0);
    f32x16 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.0f;
    for (int it = 0; it < nk; ++it) {
        store_tiles();
        if (it + 1 < nk) load_tiles(it + 1);
        lds_barrier();
        const bf16_t* bx = sa + (w * 32 + c) * TR_LS + 8 * h;
        const bf16_t* bw = sb + c * TR_LS + 8 * h;
        const int left = R - it * TR_BK;
        const int steps = left >= TR_BK ? TR_BK / 16 : (left + 15) / 16;
        for (int ks = 0; ks < steps; ++ks) {
            const bf16x8 b = lds8(bx + 16 * ks);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) mma16(acc[ct], lds8(bw + ct * 32 * TR_LS + 16 * ks), b);
        }
        lds_barrier();
    }
    // v = bf16((t pscale[k]) 0.25) once per pooled pixel; the four input pixels differ in their masks alone
    bf16_t* so = reinterpret_cast<bf16_t*>(smem_raw) + w * 32 * OS;     // the tile buffers are idle now
    tr_stage<CT, true>(acc, so, otab, c, h);
    constexpr int CPP = BO / 8;                          // 16-byte chunks per pixel
    const size_t d01 = (size_t)O, d10 = (size_t)W * (size_t)O;
#pragma unroll 2
    for (int i = 0; i < 32 * CPP / 64; ++i) {
        const int id = lane + 64 * i, px = id / CPP, ch = id - px * CPP;
        const u32x4 t = *reinterpret_cast<const u32x4*>(so + px * OS + ch * 8);
        const int mm = m0 + w * 32 + px, n = o0 + ch * 8;
        const bool ok = mm < M && n < O;                 // O % 8 == 0: the eight channels are in or out together
        // a row past M holds the window of row M - 1, a chunk past O reads channel 0: in range, and not stored
        const size_t off = (size_t)swin[w * 32 + px] * (size_t)O + (size_t)(n < O ? n : 0);
        const bf16_t* xp = xin + off;
        u32x4 xr[4];
        xr[0] = *reinterpret_cast<const u32x4*>(xp);
        xr[1] = *reinterpret_cast<const u32x4*>(xp + d01);
        xr[2] = *reinterpret_cast<const u32x4*>(xp + d10);
        xr[3] = *reinterpret_cast<const u32x4*>(xp + d10 + d01);
        float ps[8], pb[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            ps[e] = otab[ch * 8 + e];
            pb[e] = otab[BO + ch * 8 + e];
        }
        u32x4 o4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float xv[8];
            unpack8(xr[j], xv);
            o4[j] = t;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned lo = tr_pre(xv[2 * k], ps[2 * k], pb[2 * k]) > 0.0f ? 0x0000ffffu : 0u;
                const unsigned hi = tr_pre(xv[2 * k + 1], ps[2 * k + 1], pb[2 * k + 1]) > 0.0f ? 0xffff0000u : 0u;
                o4[j][k] &= lo | hi;                     // the forward's branch; elsewhere +0
            }
        }
        if (ok) {
            bf16_t* op = out + off;
            *reinterpret_cast<u32x4*>(op) = o4[0];
            *reinterpret_cast<u32x4*>(op + d01) = o4[1];
            *reinterpret_cast<u32x4*>(op + d10) = o4[2];
            *reinterpret_cast<u32x4*>(op + d10 + d01) = o4[3];
        }
    }
}

inline bool tr_dims_ok(int B, int H, int W, int K, int N) {
    return B >= 1 && H >= 2 && W >= 2 && (H % 2) == 0 && (W % 2) == 0 && K >= 8 && N >= 8 && K <= TR_MAXC && N <= TR_MAXC &&
           (K % 8) == 0 && (N % 8) == 0 && (long long)B * H * W < (1ll << 31);
}

template <int CT>
constexpr size_t tr_tile_bytes() {
    constexpr int BO = 32 * CT;
    constexpr size_t tiles = (size_t)(TR_BM + BO) * TR_LS * sizeof(bf16_t), trans = (size_t)4 * 32 * (BO + 8) * sizeof(bf16_t);
    return tiles > trans ? tiles : trans;                // a multiple of 16 either way
}

template <int CT>
void tr_launch_fwd(const bf16_t* x, const float* ps, const float* pb, const bf16_t* w, bf16_t* y, int M, int K, int N, int Wo,
                   int W, int OT, hipStream_t s) {
    constexpr size_t tab_off = tr_tile_bytes<CT>();
    // widest case (CT = 5, K = 2048): 43008 B of transposed output + 16384 B of tables
    static_assert(tab_off % 16 == 0 && tab_off + 2 * TR_MAXC * sizeof(float) <= 65536, "tiles + tables must fit 64 KiB of LDS");
    const int MT = (M + TR_BM - 1) / TR_BM, RP = (K + TR_BK - 1) / TR_BK * TR_BK;
    hipLaunchKernelGGL((tr_fwd_kernel<CT>), dim3((unsigned)MT * (unsigned)OT), dim3(256), tab_off + (size_t)2 * RP * sizeof(float),
                       s, x, ps, pb, w, y, M, K, N, Wo, W, MT, OT, (int)tab_off);
}

template <int CT>
void tr_launch_bwd(const bf16_t* g, int ldg, const bf16_t* wt, const bf16_t* xin, const float* ps, const float* pb, bf16_t* gx,
                   int M, int K, int N, int Wo, int W, int OT, hipStream_t s) {
    constexpr size_t bytes = tr_tile_bytes<CT>();
    static_assert(bytes + 2 * 32 * CT * sizeof(float) + TR_BM * sizeof(int) <= 65536, "tiles + otab + swin must fit 64 KiB of LDS");
    const int MT = (M + TR_BM - 1) / TR_BM;
    hipLaunchKernelGGL((tr_bwd_kernel<CT>), dim3((unsigned)MT * (unsigned)OT), dim3(256), bytes, s, g, wt, xin, ps, pb, gx, M, N,
                       K, Wo, W, MT, OT, ldg);
}

}  // namespace

extern "C" int adil_dense_transition_fwd(const void* x, const float* pscale, const float* pshift, const void* w, void* y,
                                         int B, int H, int W, int K, int N, void* stream) {
    if (x == nullptr || pscale == nullptr || pshift == nullptr || w == nullptr || y == nullptr || !tr_dims_ok(B, H, W, K, N))
        return ADIL_EINVAL;
    if (!aligned(x, 16) || !aligned(w, 16) || !aligned(y, 16) || !aligned(pscale, 4) || !aligned(pshift, 4)) return ADIL_EINVAL;
    ADIL_ENTER();
    const int Wo = W / 2, M = B * (H / 2) * Wo;
    // fewest channel tiles of at most 160 channels that cover N, and the narrowest tile that does it (d1_dispatch)
    const int OT = (N + 159) / 160, per = (N + OT - 1) / OT, ct = (per + 31) / 32;
    const bf16_t *xp = (const bf16_t*)x, *wp = (const bf16_t*)w;
    bf16_t* yp = (bf16_t*)y;
    hipStream_t s = (hipStream_t)stream;
    switch (ct) {
        case 1: tr_launch_fwd<1>(xp, pscale, pshift, wp, yp, M, K, N, Wo, W, OT, s); break;
        case 2: tr_launch_fwd<2>(xp, pscale, pshift, wp, yp, M, K, N, Wo, W, OT, s); break;
        case 3: tr_launch_fwd<3>(xp, pscale, pshift, wp, yp, M, K, N, Wo, W, OT, s); break;
        case 4: tr_launch_fwd<4>(xp, pscale, pshift, wp, yp, M, K, N, Wo, W, OT, s); break;
        default: tr_launch_fwd<5>(xp, pscale, pshift, wp, yp, M, K, N, Wo, W, OT, s); break;
    }
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_dense_transition_bwd(const void* g, int ldg, const void* wt, const void* xin, const float* pscale,
                                         const float* pshift, void* gx, int B, int H, int W, int K, int N, void* stream) {
    if (g == nullptr || wt == nullptr || xin == nullptr || pscale == nullptr || pshift == nullptr || gx == nullptr ||
        !tr_dims_ok(B, H, W, K, N) || ldg < N || (ldg % 8) != 0)
        return ADIL_EINVAL;
    if (!aligned(g, 16) || !aligned(wt, 16) || !aligned(xin, 16) || !aligned(gx, 16) || !aligned(pscale, 4) || !aligned(pshift, 4))
        return ADIL_EINVAL;
    ADIL_ENTER();
    const int Wo = W / 2, M = B * (H / 2) * Wo;
    const int OT = (K + 159) / 160, per = (K + OT - 1) / OT, ct = (per + 31) / 32;
    const bf16_t *gp = (const bf16_t*)g, *wp = (const bf16_t*)wt, *xp = (const bf16_t*)xin;
    bf16_t* op = (bf16_t*)gx;
    hipStream_t s = (hipStream_t)stream;
    switch (ct) {
        case 1: tr_launch_bwd<1>(gp, ldg, wp, xp, pscale, pshift, op, M, K, N, Wo, W, OT, s); break;
        case 2: tr_launch_bwd<2>(gp, ldg, wp, xp, pscale, pshift, op, M, K, N, Wo, W, OT, s); break;
        case 3: tr_launch_bwd<3>(gp, ldg, wp, xp, pscale, pshift, op, M, K, N, Wo, W, OT, s); break;
        case 4: tr_launch_bwd<4>(gp, ldg, wp, xp, pscale, pshift, op, M, K, N, Wo, W, OT, s); break;
        default: tr_launch_bwd<5>(gp, ldg, wp, xp, pscale, pshift, op, M, K, N, Wo, W, OT, s); break;
    }
    ADIL_CHECK_LAUNCH();
    return 0;
}
