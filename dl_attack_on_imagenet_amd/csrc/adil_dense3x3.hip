// 3x3 / stride 1 / pad 1 convolutions with 32-channel granularity on either side — the 128 -> 32 growth convolution
// behind every dense layer of the frozen DenseNet-121 — forward and input gradient: adil_dense3x3_fwd /
// adil_dense3x3_bwd (include/adil_hip.h).  bf16 channels_last storage, raw output (no epilogue), bf16 MFMA with fp32
// accumulation, one rounding to bf16 (RNE), no atomics, 64-bit element offsets.  A sibling of conv3x3_kernel
// (adil_conv3x3.hip), which needs 64 channels on both sides and stays as it is.
//
// Both directions are the implicit GEMM
//     OUT[m][o] = sum_{tap, r} SRC[m + (kh-1)*W + (kw-1)][r] * WP[o][tap][r]      (taps leaving the image are SELECTED away)
//   forward    SRC = x, R = C, WP = wp [N][9][C], O = N
//   gradient   SRC = g, R = N, WP = wp_bwd [C][9][N] (taps flipped on the host), O = C
// on one kernel template; the two differ only in the output tile the host picks.
//   Workgroup = 4 waves = 256 LINEARLY tiled pixels (any H, W <= 63) x BO output channels, BO = 32 CT: CT = 2 where
//   O % 64 == 0 (the gradient's 128 channels are two tiles that share their g halo in L2), else CT = 1 (the forward's 32
//   channels are ONE tile: x crosses HBM once).  A wave owns 64 pixels x BO channels = 2 CT accumulator tiles.
//   The reduction runs in chunks of 32 channels.  Per chunk the halo [m0 - W - 1, m0 + 256 + W + 1) x 32 channels and ALL
//   NINE taps of the weight chunk ([9][BO][32]) sit in LDS, so a chunk costs two barriers and not one per tap; the next
//   chunk waits in registers while this one is multiplied.  The fragment of a lane's pixel for tap (kh, kw) is the LDS row
//   pl + kh*W + kw.  LDS: 30720 B of halo + 23040 CT B of weights = 53760 B (CT = 1, three workgroups = 12 waves per CU)
//   or 76800 B (CT = 2, two workgroups = 8 waves per CU) of the 160 KiB.
//   A halo pixel in front of pixel 0 or behind pixel M - 1 is read at a clamped in-range address; its taps are masked.
//   A masked tap (off the image: that includes the neighbouring image of the batch) is replaced by zero bits BEFORE the
//   MFMA, so a NaN or Inf there never meets a multiplier.  A pixel past M is computed on clamped rows and not stored.
//   Row pitches (the _ld entry points): pixel m of SRC starts at src + m * ldsrc and holds R live channels, pixel m of OUT
//   at out + m * ldo and holds O; nothing at or behind the width is read or written, so either side may be a channel
//   slice of a wider channels_last buffer.  The packed weights are dense.  The plain entry points pass the widths.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adil_common.h"
#include "adil_hip.h"
#include "adil_mfma.h"
#include "adil_pw_tile.h"

namespace {

#define D3_BM 256
#define D3_BK 32
#define D3_LS (D3_BK + 8)                                  // LDS row stride (elements): 80 B = 5 x 16 B
#define D3_NPMAX (D3_BM + 2 * ADIL_DENSE3X3_MAX_W + 2)     // 384 halo pixels at the widest image
#define D3_XCH (D3_NPMAX * 4 / 256)                        // 16-byte halo chunks per thread (6)

template <int CT>
__global__ __launch_bounds__(256) void d3_kernel(const bf16_t* __restrict__ src, const bf16_t* __restrict__ wp,
                                                 bf16_t* __restrict__ out, int M, int H, int W, int R, int O, int MT,
                                                 int OT, int ldsrc, int ldo) {
    constexpr int BO = 32 * CT;
    constexpr int WROWS = 9 * BO;                          // rows of a weight chunk: tap * BO + o
    constexpr int WCH = (WROWS * 4 + 255) / 256;           // 16-byte chunks of it per thread
    constexpr int OS = BO + 8;                             // transposed-output pixel stride (elements)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sx = reinterpret_cast<bf16_t*>(smem_raw);      // [NP][D3_LS]   (later: [4][64][OS] output transpose)
    bf16_t* sw = sx + D3_NPMAX * D3_LS;                    // [9][BO][D3_LS]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    int mt, ot;
    pw_tile_order(MT, OT, mt, ot);                         // the OT channel tiles of one pixel tile share their halo in L2
    const long long m0 = (long long)mt * D3_BM;            // m0 + 255 may pass 2^31 - 1
    const int o0 = ot * BO;
    const int NP = D3_BM + 2 * W + 2;
    const int nk = R / D3_BK;

    // this lane's two pixels and the validity of their 9 taps
    int pl[2];
    unsigned vmask[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        pl[p] = w * 64 + p * 32 + c;
        const long long m = m0 + pl[p];
        const int mi = m < M ? (int)m : 0;                 // a pixel past M has no live tap
        const int ww = mi % W, hh = (mi / W) % H;
        unsigned vm = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int kh = t / 3, kw = t - 3 * kh;
            const bool ok = (m < M) && (hh + kh - 1 >= 0) && (hh + kh - 1 < H) && (ww + kw - 1 >= 0) && (ww + kw - 1 < W);
            vm |= ok ? (1u << t) : 0u;
        }
        vmask[p] = vm;
    }

    // the halo rows of this thread: clamped into [0, M - 1] (and into the halo: the surplus chunks are never stored)
    size_t xrow[D3_XCH];
#pragma unroll
    for (int i = 0; i < D3_XCH; ++i) {
        const int px = (tid + 256 * i) >> 2;
        long long gm = m0 - W - 1 + (px < NP ? px : NP - 1);
        gm = gm < 0 ? 0 : (gm >= M ? (long long)M - 1 : gm);
        xrow[i] = (size_t)gm * (size_t)ldsrc + (size_t)((tid & 3) * 8);
    }
    // the weight rows of this thread (the surplus chunks of the last round read row 0 and are never stored)
    size_t wrow[WCH];
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
        const int q = tid + 256 * i, row = q >> 2;
        const int tap = row / BO, o = row - tap * BO;
        wrow[i] = row < WROWS ? ((size_t)(o0 + o) * 9 + (size_t)tap) * (size_t)R + (size_t)((q & 3) * 8) : (size_t)0;
    }
    u32x4 xr[D3_XCH], wr[WCH];
    auto load_tiles = [&](int kc) {
#pragma unroll
        for (int i = 0; i < D3_XCH; ++i) xr[i] = *reinterpret_cast<const u32x4*>(src + xrow[i] + (size_t)kc * D3_BK);
#pragma unroll
        for (int i = 0; i < WCH; ++i) wr[i] = *reinterpret_cast<const u32x4*>(wp + wrow[i] + (size_t)kc * D3_BK);
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < D3_XCH; ++i) {
            const int q = tid + 256 * i, px = q >> 2;
            if (px < NP) *reinterpret_cast<u32x4*>(sx + px * D3_LS + (q & 3) * 8) = xr[i];
        }
#pragma unroll
        for (int i = 0; i < WCH; ++i) {
            const int q = tid + 256 * i, row = q >> 2;
            if (row < WROWS) *reinterpret_cast<u32x4*>(sw + row * D3_LS + (q & 3) * 8) = wr[i];
        }
    };

    f32x16 acc[2][CT];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[p][ct][r] = 0.0f;

    load_tiles(0);
    for (int it = 0; it < nk; ++it) {
        store_tiles();
        if (it + 1 < nk) load_tiles(it + 1);
        lds_barrier();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int kh = tap / 3, kw = tap - 3 * kh;
            const int shift = kh * W + kw;
            const bool ok0 = (vmask[0] >> tap) & 1u, ok1 = (vmask[1] >> tap) & 1u;
            const bf16_t* bw = sw + (tap * BO + c) * D3_LS + 8 * h;
#pragma unroll
            for (int ks = 0; ks < D3_BK / 16; ++ks) {
                u32x4 z0 = *reinterpret_cast<const u32x4*>(sx + (pl[0] + shift) * D3_LS + 16 * ks + 8 * h);
                u32x4 z1 = *reinterpret_cast<const u32x4*>(sx + (pl[1] + shift) * D3_LS + 16 * ks + 8 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) { z0[j] = ok0 ? z0[j] : 0u; z1[j] = ok1 ? z1[j] : 0u; }   // a selection
                const bf16x8 b0 = __builtin_bit_cast(bf16x8, z0), b1 = __builtin_bit_cast(bf16x8, z1);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const bf16x8 a = lds8(bw + ct * 32 * D3_LS + 16 * ks);
                    mma16(acc[0][ct], a, b0);
                    mma16(acc[1][ct], a, b1);
                }
            }
        }
        lds_barrier();                                     // every wave is done with this chunk's tiles
    }
    // epilogue: each wave transposes its own 64 pixels through LDS (the tile buffers are idle now), 16-byte stores.
    // lane = pixel, register quad q of tile ct = channels 32ct + 8q + 4h .. +3
    bf16_t* so = reinterpret_cast<bf16_t*>(smem_raw) + w * 64 * OS;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                u32x2 t;
                t[0] = pack2_bf16(acc[p][ct][4 * q], acc[p][ct][4 * q + 1]);
                t[1] = pack2_bf16(acc[p][ct][4 * q + 2], acc[p][ct][4 * q + 3]);
                *reinterpret_cast<u32x2*>(so + (p * 32 + c) * OS + 32 * ct + 8 * q + 4 * h) = t;
            }
    constexpr int CPP = BO / 8;                            // 16-byte chunks per pixel
#pragma unroll
    for (int i = 0; i < CPP; ++i) {
        const int id = lane + 64 * i, px = id / CPP, ch = id - px * CPP;
        const u32x4 t = *reinterpret_cast<const u32x4*>(so + px * OS + ch * 8);
        const long long mm = m0 + w * 64 + px;
        if (mm < M) *reinterpret_cast<u32x4*>(out + (size_t)mm * (size_t)ldo + (size_t)(o0 + ch * 8)) = t;
    }
}

template <int CT>
int d3_launch(const void* src, int ldsrc, const void* wp, void* out, int ldo, int M, int H, int W, int R, int O,
              hipStream_t st) {
    constexpr int BO = 32 * CT;
    constexpr size_t lds = (size_t)(D3_NPMAX + 9 * BO) * D3_LS * sizeof(bf16_t);
    static_assert((size_t)4 * 64 * (BO + 8) * sizeof(bf16_t) <= lds, "the output transpose reuses the tile buffers");
    static_assert(lds <= 160 * 1024, "halo + nine weight taps must fit the LDS of a CU");
    const int MT = (int)(((long long)M + D3_BM - 1) / D3_BM), OT = O / BO;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)d3_kernel<CT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((d3_kernel<CT>), dim3((unsigned)MT * (unsigned)OT), dim3(256), lds, st, (const bf16_t*)src,
                       (const bf16_t*)wp, (bf16_t*)out, M, H, W, R, O, MT, OT, ldsrc, ldo);
    ADIL_CHECK_LAUNCH();
    return 0;
}

// R = reduction channels, O = output channels of this direction; ldsrc / ldo = the row pitches of src / out (elements)
int d3_dispatch(const void* src, int ldsrc, const void* wp, void* out, int ldo, int B, int H, int W, int R, int O,
                void* stream) {
    if (src == nullptr || wp == nullptr || out == nullptr || B < 1 || H < 1 || W < 1 || W > ADIL_DENSE3X3_MAX_W || R < 32 ||
        O < 32 || R > 512 || O > 512 || (R % 32) != 0 || (O % 32) != 0)
        return ADIL_EINVAL;
    if (ldsrc < R || ldo < O || (ldsrc % 8) != 0 || (ldo % 8) != 0) return ADIL_EINVAL;
    if ((long long)B * H > 0x7fffffffLL) return ADIL_EINVAL;
    const long long M = (long long)B * H * W;
    if (M > 0x7fffffffLL) return ADIL_EINVAL;
    if (!aligned(src, 16) || !aligned(wp, 16) || !aligned(out, 16)) return ADIL_EINVAL;
    ADIL_ENTER();
    if (O % 64 == 0) return d3_launch<2>(src, ldsrc, wp, out, ldo, (int)M, H, W, R, O, (hipStream_t)stream);
    return d3_launch<1>(src, ldsrc, wp, out, ldo, (int)M, H, W, R, O, (hipStream_t)stream);
}

}  // namespace

extern "C" int adil_dense3x3_fwd_ld(const void* x, int ldx, const void* wp, void* y, int ldy, int B, int H, int W, int C,
                                    int N, void* stream) {
    return d3_dispatch(x, ldx, wp, y, ldy, B, H, W, C, N, stream);
}

extern "C" int adil_dense3x3_bwd_ld(const void* g, int ldg, const void* wp_bwd, void* gx, int ldgx, int B, int H, int W, int C,
                                    int N, void* stream) {
    return d3_dispatch(g, ldg, wp_bwd, gx, ldgx, B, H, W, N, C, stream);
}

extern "C" int adil_dense3x3_fwd(const void* x, const void* wp, void* y, int B, int H, int W, int C, int N, void* stream) {
    return d3_dispatch(x, C, wp, y, N, B, H, W, C, N, stream);
}

extern "C" int adil_dense3x3_bwd(const void* g, const void* wp_bwd, void* gx, int B, int H, int W, int C, int N,
                                 void* stream) {
    return d3_dispatch(g, N, wp_bwd, gx, C, B, H, W, N, C, stream);
}
