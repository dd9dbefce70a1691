// adil_conv3x3_wide.hip — the 3x3 convolutions of a frozen VGG (gfx950):
//   conv3x3_wide               3x3 / stride 1 / pad 1 implicit GEMM with 2-D pixel tiles inside one image: any width
//   bias_relu_pool2 fwd / bwd  bias + ReLU + 2x2 / stride 2 max-pool in one pass, and its input gradient from a byte index
// Contracts: include/adil_hip.h.
#include "adil_mfma.h"

// =========================================================================================================== //
// adil_conv3x3 (adil_convs.hip) tiles pixels LINEARLY, so its halo grows with the width and W stops at 63.  Here a
// workgroup owns a TH x 16 pixel tile of ONE image and stages the (TH+2) x 18 halo per 64-channel chunk; a halo pixel
// outside the image is written to LDS as ZEROS (a selection on the loaded registers: the load itself goes to the
// nearest pixel inside the same image, so no address is formed from an out-of-range index and nothing of another
// image or outside the operand is read).  No tap mask remains: the fragment of a lane's pixel (r, c) for tap
// (kh, kw) is the LDS row (r + kh) * 18 + (c + kw).  The main loop is conv3x3_kernel's (chunk -> tap -> ks, weight
// tiles requested three taps ahead and double buffered in LDS, one barrier per tap), so per accumulator the MFMAs run
// in the same order and the bits are those of adil_conv3x3 wherever both accept the shape.  Pixels of a partial tile
// at the right / bottom edge are computed and not stored.
// =========================================================================================================== //
namespace {

#define CW_LS 72                                         // LDS row pitch in bf16 (64 channels + 8: conflict-free 16-byte reads)
#define CW_TW 16                                         // tile width in pixels
#define CW_HP (CW_TW + 2)                                // halo pitch in pixels

template <int BN, int WPX>                               // WPX waves along pixels (64 each) x 4/WPX along channels
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void conv3x3_wide_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp, bf16_t* __restrict__ y, int H, int W, int C, int N,
    int TLH, int TLW, int MT, int NT) {
    constexpr int BM = WPX * 64;                         // pixels per workgroup: 128 (8 x 16) or 256 (16 x 16)
    constexpr int TH = BM / CW_TW;
    constexpr int NP = (TH + 2) * CW_HP;                 // halo pixels: 180 or 324
    constexpr int CTW = BN / 32 / (4 / WPX);             // channel tiles per wave
    constexpr int XCHK = (NP * 8 + 255) / 256;           // 16-byte halo chunks per thread
    constexpr int WCH = BN * 8 / 256;                    // 16-byte chunks of a weight tile per thread
    constexpr int OS = BN + 8;
    constexpr int SX = (NP * CW_LS > BM * OS ? NP * CW_LS : BM * OS);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sx = reinterpret_cast<bf16_t*>(smem_raw);    // [NP][CW_LS]  (later: [BM][OS] output transpose)
    bf16_t* sw = sx + ((SX + 7) & ~7);                   // [2][BN][CW_LS]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int wpx = w % WPX, wch = w / WPX;

    // the grid is folded into three dimensions (a tile count can pass 2^31 - 1): surplus workgroups leave at once
    const unsigned long long bid = (unsigned long long)blockIdx.x +
                                   (unsigned long long)gridDim.x * ((unsigned long long)blockIdx.y + (unsigned long long)gridDim.y * blockIdx.z);
    if (bid >= (unsigned long long)MT * (unsigned long long)NT) return;
    int mt, nt;
    if ((MT & 7) == 0) {                                  // the NT channel tiles of a pixel tile meet in one XCD's L2
        const int xcd = (int)(bid & 7);
        const unsigned long long j = bid >> 3;
        nt = (int)(j % (unsigned)NT);
        mt = (int)(j / (unsigned)NT) * 8 + xcd;
    } else {
        nt = (int)(bid % (unsigned)NT);
        mt = (int)(bid / (unsigned)NT);
    }
    const int tw = mt % TLW, th = (mt / TLW) % TLH, b = mt / (TLW * TLH);
    const int h0 = th * TH, w0 = tw * CW_TW, n0 = nt * BN;
    const int nci = C >> 6;

    int pl[2];                                            // this lane's two pixels of the tile, row-major (r * 16 + c)
#pragma unroll
    for (int p = 0; p < 2; ++p) pl[p] = (wpx * 2 + p) * 32 + c;

    u32x4 xr[XCHK], wr[3][WCH];                           // weight tiles are requested THREE taps ahead
    unsigned xvalid = 0;                                  // bit i: halo chunk i lies inside the image
    auto store_x = [&]() {
#pragma unroll
        for (int i = 0; i < XCHK; ++i) {
            const int q = tid + 256 * i, px = q >> 3, ch = q & 7;
            const bool in = (xvalid >> i) & 1u;
            u32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = in ? xr[i][k] : 0u;
            if (px < NP) *reinterpret_cast<u32x4*>(sx + px * CW_LS + ch * 8) = v;
        }
    };
    auto store_w = [&](int buf, const u32x4 (&r)[WCH]) {
#pragma unroll
        for (int i = 0; i < WCH; ++i) {
            const int q = tid + 256 * i, row = q >> 3, ch = q & 7;
            *reinterpret_cast<u32x4*>(sw + (buf * BN + row) * CW_LS + ch * 8) = r[i];
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
    // or more) on a uniform base that advances by C per tap and 64 per chunk.  Halo: 64-bit element offsets of the
    // pixel CLAMPED into this image (rows of any width: no 32-bit bound holds between two rows of a tile).
    const unsigned wq = (((unsigned)(n0 + (tid >> 3)) * 9u) * (unsigned)C + (unsigned)(tid & 7) * 8u) * 2u;
    const size_t wrow = (size_t)32 * 9 * C;                       // elements between a thread's weight rows (uniform)
    auto load_w = [&](unsigned ws, u32x4 (&r)[WCH]) {            // ws = tap * C + cc * 64
#pragma unroll
        for (int i = 0; i < WCH; ++i)
            r[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(wp + ws + i * wrow) + wq);
    };
    size_t xo[XCHK];
#pragma unroll
    for (int i = 0; i < XCHK; ++i) {
        int px = (tid >> 3) + 32 * i;
        px = px < NP ? px : NP - 1;
        const int hr = px / CW_HP, hc = px - hr * CW_HP;
        const int gh = h0 - 1 + hr, gw = w0 - 1 + hc;
        const bool in = gh >= 0 && gh < H && gw >= 0 && gw < W;
        xvalid |= in ? (1u << i) : 0u;
        const int ch_ = gh < 0 ? 0 : (gh >= H ? H - 1 : gh), cw_ = gw < 0 ? 0 : (gw >= W ? W - 1 : gw);
        xo[i] = (((size_t)b * H + ch_) * W + cw_) * (size_t)C + (size_t)(tid & 7) * 8;
    }
    auto load_x = [&](int cc) {
#pragma unroll
        for (int i = 0; i < XCHK; ++i) xr[i] = *reinterpret_cast<const u32x4*>(x + xo[i] + cc * 64);
    };
    const bf16_t* xl0 = sx + ((pl[0] >> 4) * CW_HP + (pl[0] & 15)) * CW_LS + 8 * h;
    const bf16_t* xl1 = sx + ((pl[1] >> 4) * CW_HP + (pl[1] & 15)) * CW_LS + 8 * h;
    const bf16_t* bwl = sw + ((wch * CTW) * 32 + c) * CW_LS + 8 * h;
    auto xrow = [&](const bf16_t* xl, int tap) -> const bf16_t* {   // a constant offset after unrolling
        const int kh = tap / 3, kw = tap - 3 * kh;
        return xl + (kh * CW_HP + kw) * CW_LS;
    };
    struct Frag {
        bf16x8 b0, b1, a[CTW];
    };
    auto read_frag = [&](Frag& f, const bf16_t* p0, const bf16_t* p1, const bf16_t* bw, int ks) {
        f.b0 = lds8(p0 + 16 * ks);
        f.b1 = lds8(p1 + 16 * ks);
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct) f.a[ct] = lds8(bw + ct * 32 * CW_LS + 16 * ks);
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
    __syncthreads();
    Frag fa, fb;                                                  // fa: ks 0 and 2, fb: ks 1 and 3
    const bf16_t* p0 = xrow(xl0, 0);
    const bf16_t* p1 = xrow(xl1, 0);
    read_frag(fa, p0, p1, bwl, 0);
    for (int cc = 0; cc < nci; ++cc) {
        const bool more = cc + 1 < nci;
        const unsigned wsc = (unsigned)cc * 64u, wsn = (unsigned)(more ? cc + 1 : cc) * 64u;   // surplus loads: clamped, never stored
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {                       // 9 = 3 x 3: the register-set rotation closes per chunk
            // on entry: sw[buf] holds this tap's tile and fa its ks = 0 fragments (in flight); wr[(tap+1) % 3] holds
            // the next tile, wr[(tap+2) % 3] the one after it (in flight), wr[tap % 3]'s tile is already in LDS
            const int buf = (cc + tap) & 1;                       // tile cc * 9 + tap
            const bf16_t* bw = bwl + buf * BN * CW_LS;
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
                p0 = xrow(xl0, (tap + 1) % 9);
                p1 = xrow(xl1, (tap + 1) % 9);
                read_frag(fa, p0, p1, bwl + (buf ^ 1) * BN * CW_LS, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            mma_frag(fb);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // epilogue: transpose through LDS (all waves share one [BM][OS] tile; the halo was last read before the final
    // barrier of the loop), 16-byte NHWC stores of the pixels inside the image
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
        const int gh = h0 + (px >> 4), gw = w0 + (px & 15);
        if (gh < H && gw < W)
            *reinterpret_cast<u32x4*>(y + ((img + gh) * W + gw) * (size_t)N + n0 + ch * 8) =
                *reinterpret_cast<const u32x4*>(sx + px * OS + ch * 8);
    }
}

template <int BN, int WPX>
int launch_conv3x3_wide(const void* x, const void* wp, void* y, int B, int H, int W, int C, int N, hipStream_t st) {
    constexpr int BM = WPX * 64, TH = BM / CW_TW, NP = (TH + 2) * CW_HP;
    constexpr int SX = (NP * CW_LS > BM * (BN + 8) ? NP * CW_LS : BM * (BN + 8));
    constexpr size_t lds = ((size_t)((SX + 7) & ~7) + (size_t)2 * BN * CW_LS) * sizeof(bf16_t);   // halo | two weight tiles
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    const int TLH = (H + TH - 1) / TH, TLW = (W + CW_TW - 1) / CW_TW;
    const long long MT = (long long)B * TLH * TLW;                 // <= B * H * W < 2^31
    const int NT = N / BN;
    const unsigned long long total = (unsigned long long)MT * (unsigned long long)NT;
    const unsigned long long gx = total < (1ull << 30) ? total : (1ull << 30);
    const unsigned long long rest = (total + gx - 1) / gx;
    const unsigned long long gy = rest < 32768ull ? rest : 32768ull;
    const unsigned long long gz = (rest + gy - 1) / gy;
    if (gz > 65535ull) return ADIL_EINVAL;                         // not reachable below 2^31 pixels and 2^31 weights
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)conv3x3_wide_kernel<BN, WPX>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((conv3x3_wide_kernel<BN, WPX>), dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(256), lds, st,
                       (const bf16_t*)x, (const bf16_t*)wp, (bf16_t*)y, H, W, C, N, TLH, TLW, (int)MT, NT);
    ADIL_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int adil_conv3x3_wide(const void* x, const void* wp, void* y, int B, int H, int W, int C, int N, void* stream) {
    ADIL_ENTER();
    if (!x || !wp || !y || !aligned(x, 16) || !aligned(wp, 16) || !aligned(y, 16) || B <= 0 || H <= 0 || W <= 0 || C <= 0 ||
        N <= 0 || (C % 64) || (N % 64))
        return ADIL_EINVAL;
    if ((long long)B * H * W > 0x7fffffffLL) return ADIL_EINVAL;
    if (9LL * C * N > 0x7fffffffLL) return ADIL_EINVAL;               // weight offsets are 32-bit element indices
    const hipStream_t st = (hipStream_t)stream;
    if (N % 128 == 0) return launch_conv3x3_wide<128, 2>(x, wp, y, B, H, W, C, N, st);   // 8 x 16 pixels x 128 channels
    return launch_conv3x3_wide<64, 4>(x, wp, y, B, H, W, C, N, st);                      // 16 x 16 pixels x 64 channels
}

// =========================================================================================================== //
// bias + ReLU + 2x2 / stride 2 max-pool behind a raw convolution output, and its input gradient.  One thread per
// (output pixel, 8 channels): four 16-byte loads, one 16-byte store of y and one 8-byte store of the winners' byte
// index; the backward reads those two and writes the four input pixels in full (zeros everywhere but the winner).
// Both are memory bound: 2 * (1 + 1/4 + 1/8) and 2 * (1/4 + 1/8 + 1) bytes per input element.
// =========================================================================================================== //
namespace {

__global__ __launch_bounds__(256) void bias_relu_pool2_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ bias,
                                                                  bf16_t* __restrict__ y, unsigned char* __restrict__ idx,
                                                                  int OH, int OW, int C8, size_t items) {
#pragma clang fp contract(off)
    for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
        const size_t op = it / (unsigned)C8;
        const int c8 = (int)(it - op * (unsigned)C8);
        const size_t orow = op / (unsigned)OW;                    // b * OH + oh
        const int ow = (int)(op - orow * (unsigned)OW);
        const size_t W = (size_t)OW * 2, C = (size_t)C8 * 8;
        const bf16_t* px = x + ((orow * 2) * W + (size_t)ow * 2) * C + (size_t)c8 * 8;
        float t[4][8], bs[8];
        unpack8(*reinterpret_cast<const u32x4*>(px), t[0]);
        unpack8(*reinterpret_cast<const u32x4*>(px + C), t[1]);
        unpack8(*reinterpret_cast<const u32x4*>(px + W * C), t[2]);
        unpack8(*reinterpret_cast<const u32x4*>(px + W * C + C), t[3]);
        if (bias) {
            const float4 b0 = *reinterpret_cast<const float4*>(bias + c8 * 8), b1 = *reinterpret_cast<const float4*>(bias + c8 * 8 + 4);
            bs[0] = b0.x, bs[1] = b0.y, bs[2] = b0.z, bs[3] = b0.w, bs[4] = b1.x, bs[5] = b1.y, bs[6] = b1.z, bs[7] = b1.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) bs[j] = 0.0f;
        }
        float o[8];
        unsigned wi[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float best = t[0][j] + bs[j];
            unsigned bi = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                const float v = t[k][j] + bs[j];
                if (v > best) best = v, bi = (unsigned)k;         // the first strictly greater than all before it
            }
            const bool dead = best <= 0.0f;
            o[j] = dead ? 0.0f : best;                            // +0 for a dead window (never -0)
            wi[j] = dead ? 4u : bi;
        }
        *reinterpret_cast<u32x4*>(y + it * 8) = pack8(o);
        u32x2 iv;
        iv[0] = wi[0] | (wi[1] << 8) | (wi[2] << 16) | (wi[3] << 24);
        iv[1] = wi[4] | (wi[5] << 8) | (wi[6] << 16) | (wi[7] << 24);
        *reinterpret_cast<u32x2*>(idx + it * 8) = iv;
    }
}

__global__ __launch_bounds__(256) void bias_relu_pool2_bwd_kernel(const bf16_t* __restrict__ g, const unsigned char* __restrict__ idx,
                                                                  bf16_t* __restrict__ gx, int OH, int OW, int C8, size_t items) {
    for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
        const size_t op = it / (unsigned)C8;
        const int c8 = (int)(it - op * (unsigned)C8);
        const size_t orow = op / (unsigned)OW;
        const int ow = (int)(op - orow * (unsigned)OW);
        const size_t W = (size_t)OW * 2, C = (size_t)C8 * 8;
        bf16_t* px = gx + ((orow * 2) * W + (size_t)ow * 2) * C + (size_t)c8 * 8;
        const u32x4 gv = *reinterpret_cast<const u32x4*>(g + it * 8);
        const u32x2 iv = *reinterpret_cast<const u32x2*>(idx + it * 8);
        u32x4 o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int d = 0; d < 4; ++d) {                         // dword d: channels 2d (low half) and 2d + 1 (high half)
                const unsigned i0 = (iv[d >> 1] >> (16 * (d & 1))) & 0xffu, i1 = (iv[d >> 1] >> (16 * (d & 1) + 8)) & 0xffu;
                o[k][d] = (i0 == (unsigned)k ? (gv[d] & 0xffffu) : 0u) | (i1 == (unsigned)k ? (gv[d] & 0xffff0000u) : 0u);
            }
        }
        *reinterpret_cast<u32x4*>(px) = o[0];
        *reinterpret_cast<u32x4*>(px + C) = o[1];
        *reinterpret_cast<u32x4*>(px + W * C) = o[2];
        *reinterpret_cast<u32x4*>(px + W * C + C) = o[3];
    }
}

// the shared argument check; *items = (output pixel, 8-channel group) pairs
bool pool2_covers(int B, int H, int W, int C, size_t* items) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (H & 1) || (W & 1) || (C % 8)) return false;
    if ((long long)B * H * W > 0x7fffffffLL) return false;
    *items = (size_t)B * (H / 2) * (W / 2) * (size_t)(C / 8);
    return true;
}

unsigned pool2_grid(size_t items) {
    const size_t g = (items + 255) / 256;
    return (unsigned)(g < ((size_t)1 << 20) ? g : ((size_t)1 << 20));   // the kernels stride over the rest
}

}  // namespace

extern "C" int adil_bias_relu_pool2_fwd(const void* x, const float* bias, void* y, void* idx, int B, int H, int W, int C,
                                        void* stream) {
    ADIL_ENTER();
    size_t items = 0;
    if (!x || !y || !idx || !aligned(x, 16) || !aligned(bias, 16) || !aligned(y, 16) || !aligned(idx, 8) ||
        !pool2_covers(B, H, W, C, &items))
        return ADIL_EINVAL;
    hipLaunchKernelGGL(bias_relu_pool2_fwd_kernel, dim3(pool2_grid(items)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                       bias, (bf16_t*)y, (unsigned char*)idx, H / 2, W / 2, C / 8, items);
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_bias_relu_pool2_bwd(const void* g, const void* idx, void* gx, int B, int H, int W, int C, void* stream) {
    ADIL_ENTER();
    size_t items = 0;
    if (!g || !idx || !gx || !aligned(g, 16) || !aligned(idx, 8) || !aligned(gx, 16) || !pool2_covers(B, H, W, C, &items))
        return ADIL_EINVAL;
    hipLaunchKernelGGL(bias_relu_pool2_bwd_kernel, dim3(pool2_grid(items)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)g,
                       (const unsigned char*)idx, (bf16_t*)gx, H / 2, W / 2, C / 8, items);
    ADIL_CHECK_LAUNCH();
    return 0;
}
