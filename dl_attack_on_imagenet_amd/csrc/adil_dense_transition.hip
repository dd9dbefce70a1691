// The transitions of the frozen DenseNet-121 — BatchNorm + ReLU, 1x1 convolution, AvgPool2d(2, 2) — with the pooling moved
// IN FRONT of the convolution (the two commute: both are linear and the 1x1 convolution is per pixel), forward and input
// gradient: adil_dense_transition_fwd / adil_dense_transition_bwd (include/adil_hip.h).  The GEMM runs on a quarter of the
// pixels and the full-resolution convolution output never exists.  bf16 channels_last storage, bf16 MFMA with fp32
// accumulation, one rounding to bf16 (RNE), no atomics, 64-bit element offsets.  The tile, its tails and the MFMA roles are
// those of adil_pw_tile.h; this file has what is the two kernels' own.
//
// Both directions are the GEMM  OUT[M][O] = A'[M][R] . B[O][R]^T  of adil_pw_tile.h with M = B H/2 W/2 POOLED pixels.  Pooled
// pixel mo = (b Ho + oh) Wo + ow owns the input pixels p00 = 2 (mo / Wo) W + 2 (mo % Wo), p00 + 1, p00 + W, p00 + W + 1
// (b H W + 2 oh W = 2 W (b Ho + oh): the image index needs no division of its own).
//   forward    A' = a = bf16(0.25 (((p00 + p01) + p10) + p11)), p = max(pre, 0) in fp32, pre = pw_preact's two roundings,
//              formed on the way from registers to LDS: the four input rows of a pooled pixel are gathered into registers
//              together (16 x 16 bytes in flight per thread, one chunk ahead of the MFMAs);  R = K, B = w [N][K], O = N;
//              the epilogue is the rounding alone
//   gradient   A' = g as stored, rows at a pitch of ldg;  R = N, B = wt [K][N], O = K;  epilogue: v = bf16((t pscale[k])
//              0.25) goes through LDS ONCE per pooled pixel, and on the way out each of the four input pixels keeps v
//              where its own pre > 0 and writes +0 elsewhere.  xin is fetched there, in the 16-byte chunks of the stores
//              (nothing of it is held under the reduction loop), and pre is recomputed by the forward's two operations.
//   A pooled row past M reads the window of row M - 1 and is not stored; a table entry past its extent is read at a
//   clamped index.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adil_common.h"
#include "adil_hip.h"
#include "adil_mfma.h"
#include "adil_pw_tile.h"

namespace {

// first input pixel of the window of pooled pixel mo
__device__ __forceinline__ size_t tr_p00(int mo, int Wo, int W) {
    const int r = mo / Wo, ow = mo - r * Wo;
    return (size_t)2 * (size_t)r * (size_t)W + (size_t)(2 * ow);
}

template <int CT>
__global__ __launch_bounds__(256) void tr_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ pscale,
                                                     const float* __restrict__ pshift, const bf16_t* __restrict__ bm,
                                                     bf16_t* __restrict__ out, int M, int R, int O, int Wo, int W, int MT,
                                                     int OT, int tab_off) {
    constexpr int BO = 32 * CT, ACH = PW_ACH;           // each 16-byte chunk of the A tile comes from 4 pixels
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sa = reinterpret_cast<bf16_t*>(smem_raw);    // [128][PW_LS]
    bf16_t* sb = sa + PW_BM * PW_LS;                     // [BO][PW_LS]
    float* rtab = reinterpret_cast<float*>(smem_raw + tab_off);          // pscale | pshift, zeros behind R
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    int mt, ot;
    pw_tile_order(MT, OT, mt, ot);
    const int m0 = mt * PW_BM, o0 = ot * BO;
    const int nk = (R + PW_BK - 1) / PW_BK, RP = nk * PW_BK;
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
    const PwBTile<CT> bt{br, bm, sb, o0, O, R, tid};
    auto load_tiles = [&](int kc) {
        bool cok;
        const int colc = bt.column(kc, cok);
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
        bt.load(cok, colc);
    };
    auto store_tiles = [&](int kc) {
        const int ch = tid & 7;
        const float* t0 = rtab + kc * PW_BK + ch * 8;
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
                    const float pre = pw_preact(v[e], t0[e], t0[RP + e]);
                    const float p = pre > 0.0f ? pre : 0.0f;             // <= 0 (and -0.0, and NaN) -> +0
                    s[e] = j == 0 ? p : s[e] + p;                        // ((p00 + p01) + p10) + p11
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] *= 0.25f;
            *reinterpret_cast<u32x4*>(sa + row * PW_LS + ch * 8) = pack8(s);
        }
        bt.store();
    };

    load_tiles(0);
    f32x16 acc[CT];
    pw_clear(acc);
    for (int it = 0; it < nk; ++it) {
        store_tiles(it);
        if (it + 1 < nk) load_tiles(it + 1);
        lds_barrier();
        pw_mma_chunk<CT>(acc, sa, sb, R - it * PW_BK, w, c, h);
        lds_barrier();
    }
    bf16_t* so = pw_stage_buffer<CT>(smem_raw, w);
    pw_stage<CT>(acc, so, c, h, [](float (&)[4], int, int, int) {});     // the epilogue is the rounding alone
    pw_write_out<CT>(so, out, O, m0, o0, M, O, w, lane);
}

template <int CT>
__global__ __launch_bounds__(256) void tr_bwd_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ bm,
                                                     const bf16_t* __restrict__ xin, const float* __restrict__ pscale,
                                                     const float* __restrict__ pshift, bf16_t* __restrict__ out, int M, int R,
                                                     int O, int Wo, int W, int MT, int OT, int ldg) {
    constexpr int BO = 32 * CT, ACH = PW_ACH, OS = BO + 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sa = reinterpret_cast<bf16_t*>(smem_raw);    // [128][PW_LS]
    bf16_t* sb = sa + PW_BM * PW_LS;                     // [BO][PW_LS]
    __shared__ __attribute__((aligned(16))) float otab[2 * BO];          // pscale | pshift of this channel tile
    __shared__ int swin[PW_BM];                          // first input pixel of each pooled row's window (< 2^31)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    int mt, ot;
    pw_tile_order(MT, OT, mt, ot);
    const int m0 = mt * PW_BM, o0 = ot * BO;
    const int nk = (R + PW_BK - 1) / PW_BK;
    if (tid < BO) {
        const int n = o0 + tid < O ? o0 + tid : O - 1;
        otab[tid] = pscale[n];
        otab[BO + tid] = pshift[n];
    }
    if (tid < PW_BM) swin[tid] = (int)tr_p00(m0 + tid < M ? m0 + tid : M - 1, Wo, W);
    __syncthreads();

    size_t arow[ACH];
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
        const int row = (tid + 256 * i) >> 3;
        arow[i] = (size_t)((m0 + row < M) ? m0 + row : M - 1) * (size_t)ldg;
    }
    u32x4 ar[ACH], br[CT];
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const PwBTile<CT> bt{br, bm, sb, o0, O, R, tid};
    auto load_tiles = [&](int kc) {
        bool cok;
        const int colc = bt.column(kc, cok);
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            ar[i] = *reinterpret_cast<const u32x4*>(g + arow[i] + colc);
            if (!cok) ar[i] = zero4;
        }
        bt.load(cok, colc);
    };
    auto store_tiles = [&](int) {
        const int ch = tid & 7;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int row = (tid + 256 * i) >> 3;
            *reinterpret_cast<u32x4*>(sa + row * PW_LS + ch * 8) = ar[i];
        }
        bt.store();
    };

    load_tiles(0);
    f32x16 acc[CT];
    pw_clear(acc);
    for (int it = 0; it < nk; ++it) {
        store_tiles(it);
        if (it + 1 < nk) load_tiles(it + 1);
        lds_barrier();
        pw_mma_chunk<CT>(acc, sa, sb, R - it * PW_BK, w, c, h);
        lds_barrier();
    }
    // v = bf16((t pscale[k]) 0.25) once per pooled pixel; the four input pixels differ in their masks alone
    bf16_t* so = pw_stage_buffer<CT>(smem_raw, w);
    pw_stage<CT>(acc, so, c, h, [&](float (&v)[4], int, int, int co) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (v[e] * otab[co + e]) * 0.25f;
    });
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
                const unsigned lo = pw_preact(xv[2 * k], ps[2 * k], pb[2 * k]) > 0.0f ? 0x0000ffffu : 0u;
                const unsigned hi = pw_preact(xv[2 * k + 1], ps[2 * k + 1], pb[2 * k + 1]) > 0.0f ? 0xffff0000u : 0u;
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

// the pooled GEMM has M = B H/2 W/2 rows
inline bool tr_dims_ok(int B, int H, int W, int K, int N) {
    return B >= 1 && H >= 2 && W >= 2 && (H % 2) == 0 && (W % 2) == 0 && (long long)B * H * W < (1ll << 31) &&
           pw_dims_ok(B * (H / 2) * (W / 2), K, N, 0);
}

}  // namespace

extern "C" int adil_dense_transition_fwd(const void* x, const float* pscale, const float* pshift, const void* w, void* y,
                                         int B, int H, int W, int K, int N, void* stream) {
    if (x == nullptr || pscale == nullptr || pshift == nullptr || w == nullptr || y == nullptr || !tr_dims_ok(B, H, W, K, N))
        return ADIL_EINVAL;
    if (!aligned(x, 16) || !aligned(w, 16) || !aligned(y, 16) || !aligned(pscale, 4) || !aligned(pshift, 4)) return ADIL_EINVAL;
    ADIL_ENTER();
    const int Wo = W / 2, M = B * (H / 2) * Wo;
    const bf16_t *xp = (const bf16_t*)x, *wp = (const bf16_t*)w;
    bf16_t* yp = (bf16_t*)y;
    hipStream_t s = (hipStream_t)stream;
    pw_dispatch(N, [&](auto ct, int OT) {
        constexpr int CT = decltype(ct)::value;
        constexpr size_t tab_off = pw_tile_bytes<CT>();
        // widest case (CT = 5, K = 2048): 43008 B of transposed output + 16384 B of tables
        static_assert(tab_off % 16 == 0 && tab_off + 2 * PW_MAXC * sizeof(float) <= 65536, "tiles + tables must fit 64 KiB of LDS");
        const int MT = pw_pixel_tiles(M), RP = (K + PW_BK - 1) / PW_BK * PW_BK;
        hipLaunchKernelGGL((tr_fwd_kernel<CT>), dim3((unsigned)MT * (unsigned)OT), dim3(256),
                           tab_off + (size_t)2 * RP * sizeof(float), s, xp, pscale, pshift, wp, yp, M, K, N, Wo, W, MT, OT,
                           (int)tab_off);
    });
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_dense_transition_bwd(const void* g, int ldg, const void* wt, const void* xin, const float* pscale,
                                         const float* pshift, void* gx, int B, int H, int W, int K, int N, void* stream) {
    if (g == nullptr || wt == nullptr || xin == nullptr || pscale == nullptr || pshift == nullptr || gx == nullptr ||
        !tr_dims_ok(B, H, W, K, N) || !pw_ld_ok(ldg, N))
        return ADIL_EINVAL;
    if (!aligned(g, 16) || !aligned(wt, 16) || !aligned(xin, 16) || !aligned(gx, 16) || !aligned(pscale, 4) || !aligned(pshift, 4))
        return ADIL_EINVAL;
    ADIL_ENTER();
    const int Wo = W / 2, M = B * (H / 2) * Wo;
    const bf16_t *gp = (const bf16_t*)g, *wp = (const bf16_t*)wt, *xp = (const bf16_t*)xin;
    bf16_t* op = (bf16_t*)gx;
    hipStream_t s = (hipStream_t)stream;
    pw_dispatch(K, [&](auto ct, int OT) {
        constexpr int CT = decltype(ct)::value;
        constexpr size_t bytes = pw_tile_bytes<CT>();
        static_assert(bytes + 2 * 32 * CT * sizeof(float) + PW_BM * sizeof(int) <= 65536, "tiles + otab + swin must fit 64 KiB of LDS");
        const int MT = pw_pixel_tiles(M);
        hipLaunchKernelGGL((tr_bwd_kernel<CT>), dim3((unsigned)MT * (unsigned)OT), dim3(256), bytes, s, gp, wp, xp, pscale, pshift,
                           op, M, N, K, Wo, W, MT, OT, ldg);
    });
    ADIL_CHECK_LAUNCH();
    return 0;
}
