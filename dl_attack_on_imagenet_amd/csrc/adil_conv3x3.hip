// adil_conv3x3.hip — the 3x3 / stride 1 / pad 1 convolution of the frozen classifiers (conv2 of every ResNet bottleneck, the
// convolutions of a VGG behind its first group), NHWC bf16, raw output, as ONE implicit-GEMM kernel on two pixel geometries
// (gfx950):
//   adil_conv3x3        linear pixel tiles (W <= 63)
//   adil_conv3x3_wide   2-D pixel tiles inside one image (any width)
// Contracts: include/adil_hip.h.
#include <type_traits>

#include "adil_mfma.h"

// =========================================================================================================== //
// A BatchNorm / bias + ReLU lives in the next kernel, so this one is a pure implicit GEMM
//     Y[m][n] = sum_{tap, c} X[m + (kh-1)*W + (kw-1)][c] * Wp[n][tap][c]        (taps crossing an image edge are zeros)
// and the input gradient is the same kernel on flipped / transposed weights.  Per 64-channel chunk a workgroup stages the
// halo of its pixel tile in LDS once; per tap one weight tile (double buffered, the tiles of the next three taps in
// registers or in flight), ONE barrier, 16 MFMAs per wave on 64 px x 64 (32) channel wave tiles.  No zero-fill launch, no
// epilogue pass.  The two geometries differ in what a tile is and share everything behind that:
//   linear (TILE2D = false)  128 / 256 consecutive (n,h,w) indices, any H, W <= 63: the halo is the contiguous range
//       [m0-W-1, m0+BM+W+1), so it grows with the width; the fragment of a lane's pixel for tap (kh,kw) is the LDS row
//       pl + kh*W + kw, and a tap that leaves the image reads a row of zeros instead (a mask bit per lane and tap).
//   2-D (TILE2D = true)  a TH x 16 tile of ONE image and its (TH+2) x 18 halo; a halo pixel outside the image is written to
//       LDS as ZEROS (a selection on the loaded registers: the load itself goes to the nearest pixel inside the same
//       image, so no address is formed from an out-of-range index and nothing of another image or outside the operand is
//       read).  No tap mask remains: the fragment of a lane's pixel (r, c) for tap (kh, kw) is the LDS row
//       (r + kh) * 18 + (c + kw).  Pixels of a partial tile at the right / bottom edge are computed and not stored.
// Per accumulator the MFMAs run chunk -> tap -> ks in both, so the bits are the same wherever both accept the shape
// (tests/golden/retired_variant_bits.json holds the bits of that order).
// =========================================================================================================== //
namespace {

constexpr int C3_LS = 72;                                // LDS row pitch in bf16 (64 channels + 8: conflict-free 16-byte reads)
constexpr int C3_TW = 16;                                // 2-D tiles: tile width in pixels
constexpr int C3_HP = C3_TW + 2;                         // 2-D tiles: halo pitch in pixels

// the integer arguments of a geometry, in the order its kernel has always taken them; what a geometry does not take is a
// constant, so the kernel can name every field
template <bool TILE2D>
struct C3Geo {                                           // linear: M = B * H * W pixels in MT tiles
    int M, H, W, C, N, MT, NT;
    static constexpr int TLH = 1, TLW = 1;
};
template <>
struct C3Geo<true> {                                     // 2-D: TLH x TLW tiles per image, MT in all
    int H, W, C, N, TLH, TLW, MT, NT;
    static constexpr int M = 0;
};

// The main loop: a run-time loop over 64-channel chunks with the 9 taps unrolled (constant kh, kw, mask bit; one 32-bit
// weight offset per thread plus a scalar), two fragment register sets so that the LDS reads of ks + 1 fly under the MFMAs
// of ks, and the barrier between the MFMAs of ks = 2 and ks = 3: the first fragments of the next tap are read under
// ks = 3.  `if constexpr (TILE2D)` marks every place where the geometries differ; the rest is one text (the linear
// instantiations sit at 256 VGPRs: a shared piece goes in as text, not as a helper, profiles/conv3x3_one_kernel.md).
template <int BN, int WPX, bool TILE2D, typename... GEO>  // WPX waves along pixels (64 each) x 4/WPX along channels
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void conv3x3_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp, bf16_t* __restrict__ y, GEO... ints) {
    const C3Geo<TILE2D> geo = {ints...};                 // separate int arguments: each geometry keeps its kernarg layout
    constexpr int BM = WPX * 64;                         // pixels per workgroup: 128 (2 x 2 waves) or 256 (4 x 1 waves)
    constexpr int TH = BM / C3_TW;                       // 2-D tiles: 8 x 16 or 16 x 16 pixels
    constexpr int NP2D = (TH + 2) * C3_HP;               // 2-D tiles: halo pixels, 180 or 324
    constexpr int CTW = BN / 32 / (4 / WPX);             // channel tiles per wave
    // 16-byte halo chunks per thread (linear: NP <= BM + 128, W <= 63)
    constexpr int XCHK = TILE2D ? (NP2D * 8 + 255) / 256 : (BM + 128) * 8 / 256;
    constexpr int WCH = BN * 8 / 256;                    // 16-byte chunks of a weight tile per thread
    constexpr int OS = BN + 8;
    const int H = geo.H, W = geo.W, C = geo.C, N = geo.N, MT = geo.MT, NT = geo.NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int NP = TILE2D ? NP2D : BM + 2 * W + 2;       // halo pixels
    bf16_t* sx = reinterpret_cast<bf16_t*>(smem_raw);    // [NP][C3_LS]  (later: [BM][OS] output transpose)
    const int sx_elems = (NP * C3_LS > BM * OS ? NP * C3_LS : BM * OS);
    bf16_t* sw = sx + ((sx_elems + 7) & ~7);             // [2][BN][C3_LS]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int wpx = w % WPX, wch = w / WPX;

    // workgroup id -> (pixel tile mt, channel tile nt): where MT is a multiple of 8 the NT channel tiles of a pixel tile
    // meet in one XCD's L2.  2-D: the grid is folded into three dimensions (a tile count can pass 2^31 - 1) and surplus
    // workgroups leave at once; that exit stands at function scope (inside the block below hipcc loses its direct branch)
    unsigned long long bid = 0;
    if constexpr (TILE2D)
        bid = (unsigned long long)blockIdx.x +
              (unsigned long long)gridDim.x * ((unsigned long long)blockIdx.y + (unsigned long long)gridDim.y * blockIdx.z);
    if (TILE2D && bid >= (unsigned long long)MT * (unsigned long long)NT) return;
    int mt, nt;
    if constexpr (TILE2D) {
        if ((MT & 7) == 0) {
            const int xcd = (int)(bid & 7);
            const unsigned long long j = bid >> 3;
            nt = (int)(j % (unsigned)NT);
            mt = (int)(j / (unsigned)NT) * 8 + xcd;
        } else {
            nt = (int)(bid % (unsigned)NT);
            mt = (int)(bid / (unsigned)NT);
        }
    } else {
        if ((MT & 7) == 0) {
            const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
            nt = j % NT;
            mt = (j / NT) * 8 + xcd;
        } else {
            nt = blockIdx.x % NT;
            mt = blockIdx.x / NT;
        }
    }
    // linear: the tile's first pixel.  Assigned, not initialised as constants: with `const int M = geo.M, m0 = mt * BM`
    // hipcc allocates two registers of the linear instantiations the other way round (profiles/conv3x3_one_kernel.md)
    int M = 0, m0 = 0;
    if constexpr (!TILE2D) M = geo.M, m0 = mt * BM;
    const int tw = mt % geo.TLW, th = (mt / geo.TLW) % geo.TLH, b = mt / (geo.TLW * geo.TLH);   // 2-D: tile and image
    const int h0 = th * TH, w0 = tw * C3_TW, n0 = nt * BN;
    const int nci = C >> 6;

    // this lane's two pixels of the tile (2-D: row-major, r * 16 + c) and, linear, the validity of their 9 taps
    int pl[2];
    unsigned vmask[2] = {0u, 0u};
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        pl[p] = (wpx * 2 + p) * 32 + c;
        if constexpr (!TILE2D) {
            const int m = m0 + pl[p];
            const int ww = m % W, hh = (m / W) % H;
            unsigned vm = 0;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int kh = t / 3, kw = t - 3 * kh;
                const bool ok = (m < M) && (hh + kh - 1 >= 0) && (hh + kh - 1 < H) && (ww + kw - 1 >= 0) && (ww + kw - 1 < W);
                vm |= ok ? (1u << t) : 0u;
            }
            vmask[p] = vm;
        }
    }

    u32x4 xr[XCHK], wr[3][WCH];                           // weight tiles are requested THREE taps ahead (an L2 round trip
                                                          // is ~5x the 16 MFMAs of one tap)
    unsigned xvalid = 0;                                  // 2-D: bit i = halo chunk i lies inside the image
    auto store_x = [&]() {
#pragma unroll
        for (int i = 0; i < XCHK; ++i) {
            const int q = tid + 256 * i, px = q >> 3, ch = q & 7;
            if constexpr (TILE2D) {
                const bool in = (xvalid >> i) & 1u;
                u32x4 v;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = in ? xr[i][k] : 0u;
                if (px < NP) *reinterpret_cast<u32x4*>(sx + px * C3_LS + ch * 8) = v;
            } else {
                if (px < NP) *reinterpret_cast<u32x4*>(sx + px * C3_LS + ch * 8) = xr[i];
            }
        }
    };
    auto store_w = [&](int buf, const u32x4 (&r)[WCH]) {
#pragma unroll
        for (int i = 0; i < WCH; ++i) {
            const int q = tid + 256 * i, row = q >> 3, ch = q & 7;
            *reinterpret_cast<u32x4*>(sw + (buf * BN + row) * C3_LS + ch * 8) = r[i];
        }
    };

    f32x16 acc[2][CTW];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[p][ct][r] = 0.0f;

    // ---- addresses, once.  Weights: one 32-bit byte offset per thread (the launcher refuses packs of 2^31 elements
    // or more) on a uniform base that advances by C per tap and 64 per chunk.
    const unsigned wq = (((unsigned)(n0 + (tid >> 3)) * 9u) * (unsigned)C + (unsigned)(tid & 7) * 8u) * 2u;
    const size_t wrow = (size_t)32 * 9 * C;                       // elements between a thread's weight rows (uniform)
    auto load_w = [&](unsigned ws, u32x4 (&r)[WCH]) {            // ws = tap * C + cc * 64
#pragma unroll
        for (int i = 0; i < WCH; ++i)
            r[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(wp + ws + i * wrow) + wq);
    };
    // Halo, linear: 32-bit byte offsets from the tile's first halo row (at most BM + 128 rows of C elements: far below
    // 2^32 bytes wherever the pack fits), the pixel clamped into [0, M-1].  2-D: 64-bit element offsets of the pixel
    // CLAMPED into this image (rows of any width: no 32-bit bound holds between two rows of a tile).
    std::conditional_t<TILE2D, size_t, unsigned> xo[XCHK];
    const bf16_t* xb = x;
    if constexpr (TILE2D) {
#pragma unroll
        for (int i = 0; i < XCHK; ++i) {
            int px = (tid >> 3) + 32 * i;
            px = px < NP ? px : NP - 1;
            const int hr = px / C3_HP, hc = px - hr * C3_HP;
            const int gh = h0 - 1 + hr, gw = w0 - 1 + hc;
            const bool in = gh >= 0 && gh < H && gw >= 0 && gw < W;
            xvalid |= in ? (1u << i) : 0u;
            const int ch_ = gh < 0 ? 0 : (gh >= H ? H - 1 : gh), cw_ = gw < 0 ? 0 : (gw >= W ? W - 1 : gw);
            xo[i] = (((size_t)b * H + ch_) * W + cw_) * (size_t)C + (size_t)(tid & 7) * 8;
        }
    } else {
        const int gmb = m0 - W - 1 > 0 ? m0 - W - 1 : 0;
        xb = x + (size_t)gmb * C;
#pragma unroll
        for (int i = 0; i < XCHK; ++i) {
            const int px = (tid >> 3) + 32 * i;
            int gm = m0 - W - 1 + (px < NP ? px : NP - 1);
            gm = gm < 0 ? 0 : (gm >= M ? M - 1 : gm);
            xo[i] = ((unsigned)(gm - gmb) * (unsigned)C + (unsigned)(tid & 7) * 8u) * 2u;
        }
    }
    auto load_x = [&](int cc) {
#pragma unroll
        for (int i = 0; i < XCHK; ++i) {
            if constexpr (TILE2D) xr[i] = *reinterpret_cast<const u32x4*>(x + xo[i] + cc * 64);
            else xr[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(xb + cc * 64) + xo[i]);
        }
    };
    bf16_t* sz = sw + 2 * BN * C3_LS;                             // linear: [C3_LS] zeros, what a tap outside the image reads
    auto lrow = [&](int p) { return TILE2D ? (pl[p] >> 4) * C3_HP + (pl[p] & 15) : pl[p]; };   // a lane's pixel in the halo
    const bf16_t* xl0 = sx + lrow(0) * C3_LS + 8 * h;
    const bf16_t* xl1 = sx + lrow(1) * C3_LS + 8 * h;
    const bf16_t* zl = sz + 8 * h;
    const bf16_t* bwl = sw + ((wch * CTW) * 32 + c) * C3_LS + 8 * h;
    // the LDS row of pixel p's fragment at a tap (a constant offset after unrolling).  Linear: a lane past M computes a
    // row that is never written, so the centre tap, which never leaves the image, takes no select
    auto xrow = [&](const bf16_t* xl, unsigned vm, int tap) -> const bf16_t* {
        const int kh = tap / 3, kw = tap - 3 * kh;
        if constexpr (TILE2D) {
            return xl + (kh * C3_HP + kw) * C3_LS;
        } else {
            const bf16_t* a = xl + (kh * W + kw) * C3_LS;
            if (tap == 4) return a;
            return (vm & (1u << tap)) ? a : zl;
        }
    };
    struct Frag {
        bf16x8 b0, b1, a[CTW];
    };
    auto read_frag = [&](Frag& f, const bf16_t* p0, const bf16_t* p1, const bf16_t* bw, int ks) {
        f.b0 = lds8(p0 + 16 * ks);
        f.b1 = lds8(p1 + 16 * ks);
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct) f.a[ct] = lds8(bw + ct * 32 * C3_LS + 16 * ks);
    };
    auto mma_frag = [&](const Frag& f) {
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct) {
            mma16(acc[0][ct], f.a[ct], f.b0);
            mma16(acc[1][ct], f.a[ct], f.b1);
        }
    };

    load_x(0);
    load_w(0u, wr[0]);
    load_w((unsigned)C, wr[1]);
    load_w(2u * (unsigned)C, wr[2]);
    store_x();
    store_w(0, wr[0]);
    if constexpr (!TILE2D)
        if (tid < C3_LS / 8) reinterpret_cast<u32x4*>(sz)[tid] = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    Frag fa, fb;                                                  // fa: ks 0 and 2, fb: ks 1 and 3
    const bf16_t* p0 = xrow(xl0, vmask[0], 0);
    const bf16_t* p1 = xrow(xl1, vmask[1], 0);
    read_frag(fa, p0, p1, bwl, 0);
    for (int cc = 0; cc < nci; ++cc) {
        const bool more = cc + 1 < nci;
        const unsigned wsc = (unsigned)cc * 64u, wsn = (unsigned)(more ? cc + 1 : cc) * 64u;   // surplus loads: clamped, never stored
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {                       // 9 = 3 x 3: the register-set rotation closes per chunk
            // on entry: sw[buf] holds this tap's tile and fa its ks = 0 fragments (in flight); wr[(tap+1) % 3] holds
            // the next tile, wr[(tap+2) % 3] the one after it (in flight), wr[tap % 3]'s tile is already in LDS
            const int buf = (cc + tap) & 1;                       // tile cc * 9 + tap
            const bf16_t* bw = bwl + buf * BN * C3_LS;
            const bool last = !more && tap == 8;
            read_frag(fb, p0, p1, bw, 1);
            if (!last) store_w(buf ^ 1, wr[(tap + 1) % 3]);       // read last before the previous barrier
            load_w(tap + 3 < 9 ? wsc + (unsigned)((tap + 3) * C) : wsn + (unsigned)((tap - 6) * C), wr[tap % 3]);
            if (tap == 4 && more) load_x(cc + 1);                // next channel chunk's halo flies under taps 4..8
            __builtin_amdgcn_sched_barrier(0);
            mma_frag(fa);
            __builtin_amdgcn_sched_barrier(0);
            read_frag(fa, p0, p1, bw, 2);
            __builtin_amdgcn_sched_barrier(0);
            mma_frag(fb);
            __builtin_amdgcn_sched_barrier(0);
            read_frag(fb, p0, p1, bw, 3);
            __builtin_amdgcn_sched_barrier(0);
            mma_frag(fa);
            __builtin_amdgcn_sched_barrier(0);
            // every wave has read all of this tap's fragments and written the next tile: the barrier sits under
            // the MFMAs of ks = 3, and so do the first reads of the next tap
            lds_barrier();
            if (tap == 8 && more) {                               // all waves are done with this halo
                store_x();
                lds_barrier();
            }
            if (!last) {
                p0 = xrow(xl0, vmask[0], (tap + 1) % 9);
                p1 = xrow(xl1, vmask[1], (tap + 1) % 9);
                read_frag(fa, p0, p1, bwl + (buf ^ 1) * BN * C3_LS, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            mma_frag(fb);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // epilogue: transpose through LDS (all waves share one [BM][OS] tile; the halo was last read before the final
    // barrier of the loop), 16-byte NHWC stores of the pixels that exist
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                u32x2 t;
                t[0] = pack2_bf16(acc[p][ct][4 * q], acc[p][ct][4 * q + 1]);
                t[1] = pack2_bf16(acc[p][ct][4 * q + 2], acc[p][ct][4 * q + 3]);
                *reinterpret_cast<u32x2*>(sx + pl[p] * OS + (wch * CTW + ct) * 32 + 8 * q + 4 * h) = t;
            }
        }
    }
    __syncthreads();
    constexpr int CPP = BN / 8;
    const size_t img = (size_t)b * H;
#pragma unroll
    for (int i = 0; i < BM * CPP / 256; ++i) {
        const int id = tid + 256 * i, px = id / CPP, ch = id - px * CPP;
        if constexpr (TILE2D) {
            const int gh = h0 + (px >> 4), gw = w0 + (px & 15);
            if (gh < H && gw < W)
                *reinterpret_cast<u32x4*>(y + ((img + gh) * W + gw) * (size_t)N + n0 + ch * 8) =
                    *reinterpret_cast<const u32x4*>(sx + px * OS + ch * 8);
        } else {
            const int mm = m0 + px;
            if (mm < M) *reinterpret_cast<u32x4*>(y + (size_t)mm * N + n0 + ch * 8) = *reinterpret_cast<const u32x4*>(sx + px * OS + ch * 8);
        }
    }
}

// B * H * W <= 2^31 - 1 and 9 * C * N <= 2^31 - 1 are the entry points' to check
template <int BN, int WPX, bool TILE2D>
int launch_conv3x3(const void* x, const void* wp, void* y, int B, int H, int W, int C, int N, hipStream_t st) {
    constexpr int BM = WPX * 64, TH = BM / C3_TW;
    const int NP = TILE2D ? (TH + 2) * C3_HP : BM + 2 * W + 2;
    size_t sx_elems = (size_t)NP * C3_LS;
    if (sx_elems < (size_t)BM * (BN + 8)) sx_elems = (size_t)BM * (BN + 8);
    sx_elems = (sx_elems + 7) & ~(size_t)7;
    // halo | two weight tiles | linear: the row of zeros
    const size_t lds = (sx_elems + (size_t)2 * BN * C3_LS + (TILE2D ? 0 : C3_LS)) * sizeof(bf16_t);
    if (lds > (TILE2D ? 80 : 160) * 1024) return ADIL_EINVAL;      // 2-D: two workgroups per CU, whatever the shape
    const int NT = N / BN;
    auto launch = [&](dim3 grid, auto... ints) -> int {             // the geometry's integers, in the order of its C3Geo
        const auto kernel = conv3x3_kernel<BN, WPX, TILE2D, decltype(ints)...>;
        if (lds > 48 * 1024) {
            const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return (int)e;
        }
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, (const bf16_t*)x, (const bf16_t*)wp, (bf16_t*)y, ints...);
        ADIL_CHECK_LAUNCH();
        return 0;
    };
    if constexpr (TILE2D) {
        const int TLH = (H + TH - 1) / TH, TLW = (W + C3_TW - 1) / C3_TW;
        const long long MT = (long long)B * TLH * TLW;             // <= B * H * W < 2^31
        const unsigned long long total = (unsigned long long)MT * (unsigned long long)NT;
        const unsigned long long gx = total < (1ull << 30) ? total : (1ull << 30);
        const unsigned long long rest = (total + gx - 1) / gx;
        const unsigned long long gy = rest < 32768ull ? rest : 32768ull;
        const unsigned long long gz = (rest + gy - 1) / gy;
        if (gz > 65535ull) return ADIL_EINVAL;                     // not reachable below 2^31 pixels and 2^31 weights
        return launch(dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), H, W, C, N, TLH, TLW, (int)MT, NT);
    } else {
        const int M = B * H * W, MT = (M + BM - 1) / BM;
        return launch(dim3((unsigned)(MT * NT)), M, H, W, C, N, MT, NT);
    }
}

}  // namespace

extern "C" int adil_conv3x3(const void* x, const void* wp, void* y, int B, int H, int W, int C, int N, void* stream) {
    ADIL_ENTER();
    if (!x || !wp || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0 || (C % 64) || (N % 64) || W > 63) return ADIL_EINVAL;   // halo = 128 + 2W + 2 pixels <= 256
    if ((long long)B * H * W > 0x7fffffffLL) return ADIL_EINVAL;
    if (9LL * C * N > 0x7fffffffLL) return ADIL_EINVAL;               // weight offsets are 32-bit element indices
    const hipStream_t st = (hipStream_t)stream;
    if (N % 128 == 0) return launch_conv3x3<128, 2, false>(x, wp, y, B, H, W, C, N, st);
    return launch_conv3x3<64, 4, false>(x, wp, y, B, H, W, C, N, st);   // 64 px x 64 ch wave tiles as well
}

extern "C" int adil_conv3x3_wide(const void* x, const void* wp, void* y, int B, int H, int W, int C, int N, void* stream) {
    ADIL_ENTER();
    if (!x || !wp || !y || !aligned(x, 16) || !aligned(wp, 16) || !aligned(y, 16) || B <= 0 || H <= 0 || W <= 0 || C <= 0 ||
        N <= 0 || (C % 64) || (N % 64))
        return ADIL_EINVAL;
    if ((long long)B * H * W > 0x7fffffffLL) return ADIL_EINVAL;
    if (9LL * C * N > 0x7fffffffLL) return ADIL_EINVAL;               // weight offsets are 32-bit element indices
    const hipStream_t st = (hipStream_t)stream;
    if (N % 128 == 0) return launch_conv3x3<128, 2, true>(x, wp, y, B, H, W, C, N, st);   // 8 x 16 pixels x 128 channels
    return launch_conv3x3<64, 4, true>(x, wp, y, B, H, W, C, N, st);                      // 16 x 16 pixels x 64 channels
}
