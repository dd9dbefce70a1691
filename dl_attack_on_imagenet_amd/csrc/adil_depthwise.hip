// Depthwise 3x3 / pad 1 / stride 1|2 convolution of the frozen network (the 17 `groups == channels` layers of
// MobileNetV2) with its folded eval-BatchNorm and ReLU6, forward and input gradient: adil_dw3x3_fwd / adil_dw3x3_bwd
// (include/adil_hip.h).  bf16 channels_last storage, fp32 arithmetic, one rounding to bf16 (RNE), no atomics.
//
// 9 MACs per output element: both kernels are HBM streams (forward 2 B C (HW + OH OW) bytes, gradient
// 2 B C (HW + 2 OH OW) bytes), so the shape is the plainest one that keeps every access a 16-byte lane:
//   - a thread owns 8 channels (one 16-byte lane of the C axis) of DW_TW = 4 neighbouring output columns of one row;
//     consecutive threads own consecutive channel groups, so a wave reads and writes contiguous runs of the C axis;
//   - per tap row it loads the S (TW - 1) + 3 input columns the four outputs share (6 at stride 1, 9 at stride 2) and
//     reuses them from registers; the 3 x 8 fp32 weights of the row come from the cache next to them.  Vertical reuse
//     (the 3 rows an input row serves) and the halo columns between neighbouring threads are left to the L2: an input
//     row of the widest layer (112 x 96 x 2 B = 21 KB) stays resident between its three uses;
//   - borders: an out-of-range column is read at a clamped address and replaced by +0 (never a branch around a single
//     load), an out-of-range row skips the whole tap row (uniform over nearly every wave);
//   - the gradient is a gather over the output grid: pixel (h, w) reads g at ((h + 1 - kh) / S, (w + 1 - kw) / S) for the
//     taps whose quotients are integers and in range — at stride 2 that is 1 or 2 rows and, for an aligned run of four
//     columns, 3 columns of g with a fixed compile-time tap pattern.  g is never zero-upsampled.  The ReLU6 mask
//     [0 < y < 6] is taken from the stored y by comparing VALUES (a -0.0 in y is a zero: masked).
// Accumulation order of one output: taps kh*3+kw ascending over the live taps, accumulator starting at +0, then the
// bias (forward).  Element offsets are 64-bit throughout (B = 2048 at 112 x 112 x 96 passes 2^31 elements).
#include "adil_common.h"

#define DW_TW 4          // output columns per thread
#define DW_THREADS 256

namespace {

struct Vec8 {
    float v[8];
};

__device__ __forceinline__ Vec8 unpack8(const uint4 u) {
    Vec8 r;
    r.v[0] = __uint_as_float(u.x << 16);
    r.v[1] = __uint_as_float(u.x & 0xffff0000u);
    r.v[2] = __uint_as_float(u.y << 16);
    r.v[3] = __uint_as_float(u.y & 0xffff0000u);
    r.v[4] = __uint_as_float(u.z << 16);
    r.v[5] = __uint_as_float(u.z & 0xffff0000u);
    r.v[6] = __uint_as_float(u.w << 16);
    r.v[7] = __uint_as_float(u.w & 0xffff0000u);
    return r;
}

__device__ __forceinline__ uint4 pack8(const float* a) {
    uint4 u;
    u.x = pack2_bf16(a[0], a[1]);
    u.y = pack2_bf16(a[2], a[3]);
    u.z = pack2_bf16(a[4], a[5]);
    u.w = pack2_bf16(a[6], a[7]);
    return u;
}

__device__ __forceinline__ Vec8 load_w8(const float* __restrict__ p) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    Vec8 r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}

// Decompose the linear work index: channel group innermost, then the column tile, the row, the image.
struct Item {
    int cg, tile, row;
    size_t img;
};
__device__ __forceinline__ Item decompose(size_t i, int CG, int tiles, int rows) {
    Item it;
    if ((i >> 32) == 0) {                 // the usual case: 32-bit division (a 64-bit one is a long software routine)
        unsigned u = (unsigned)i;
        it.cg = (int)(u % (unsigned)CG);
        u /= (unsigned)CG;
        it.tile = (int)(u % (unsigned)tiles);
        u /= (unsigned)tiles;
        it.row = (int)(u % (unsigned)rows);
        it.img = u / (unsigned)rows;
        return it;
    }
    it.cg = (int)(i % (size_t)CG);
    i /= (size_t)CG;
    it.tile = (int)(i % (size_t)tiles);
    i /= (size_t)tiles;
    it.row = (int)(i % (size_t)rows);
    it.img = i / (size_t)rows;
    return it;
}

template <int S, bool RELU6>
__global__ __launch_bounds__(DW_THREADS) void dw3x3_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, bf16_t* __restrict__ y,
                                                               int H, int W, int C, int OH, int OW, size_t total) {
    constexpr int NCOL = S * (DW_TW - 1) + 3;
    const int CG = C >> 3, tiles = (OW + DW_TW - 1) / DW_TW;
    for (size_t i = (size_t)blockIdx.x * DW_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * DW_THREADS) {
        const Item it = decompose(i, CG, tiles, OH);
        const int c0 = it.cg << 3, ow0 = it.tile * DW_TW, ic0 = S * ow0 - 1;
        float acc[DW_TW][8];
#pragma unroll
        for (int j = 0; j < DW_TW; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[j][e] = 0.0f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int ih = S * it.row - 1 + kh;
            if (ih < 0 || ih >= H) continue;
            const bf16_t* xrow = x + ((it.img * (size_t)H + (size_t)ih) * (size_t)W) * (size_t)C + c0;
            uint4 raw[NCOL];
#pragma unroll
            for (int q = 0; q < NCOL; ++q) {
                const int ic = ic0 + q;
                const int icc = min(max(ic, 0), W - 1);
                raw[q] = *reinterpret_cast<const uint4*>(xrow + (size_t)icc * (size_t)C);
                if (ic < 0 || ic >= W) raw[q] = make_uint4(0u, 0u, 0u, 0u);
            }
            Vec8 wk[3];
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) wk[kw] = load_w8(w + (size_t)(kh * 3 + kw) * (size_t)C + c0);
            Vec8 xv[NCOL];
#pragma unroll
            for (int q = 0; q < NCOL; ++q) xv[q] = unpack8(raw[q]);
#pragma unroll
            for (int j = 0; j < DW_TW; ++j)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw)           // output column ow0 + j reads input column ic0 + S j + kw
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[j][e] = fmaf(xv[S * j + kw].v[e], wk[kw].v[e], acc[j][e]);
        }
        Vec8 bv;
#pragma unroll
        for (int e = 0; e < 8; ++e) bv.v[e] = 0.0f;
        if (bias != nullptr) bv = load_w8(bias + c0);
        bf16_t* yrow = y + ((it.img * (size_t)OH + (size_t)it.row) * (size_t)OW) * (size_t)C + c0;
#pragma unroll
        for (int j = 0; j < DW_TW; ++j) {
            if (ow0 + j < OW) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float v = acc[j][e] + bv.v[e];
                    if (RELU6) v = fminf(fmaxf(v, 0.0f), 6.0f);
                    o[e] = v;
                }
                *reinterpret_cast<uint4*>(yrow + (size_t)(ow0 + j) * (size_t)C) = pack8(o);
            }
        }
    }
}

template <int S, bool RELU6>
__global__ __launch_bounds__(DW_THREADS) void dw3x3_bwd_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ y,
                                                               const float* __restrict__ w, bf16_t* __restrict__ gx,
                                                               int H, int W, int C, int OH, int OW, size_t total) {
    // columns of g an aligned run of DW_TW input columns gathers from: stride 1: w0 - 1 .. w0 + 4; stride 2: w0/2 .. w0/2 + 2
    constexpr int NCOL = (S == 1) ? DW_TW + 2 : DW_TW / 2 + 1;
    const int CG = C >> 3, tiles = (W + DW_TW - 1) / DW_TW;
    for (size_t i = (size_t)blockIdx.x * DW_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * DW_THREADS) {
        const Item it = decompose(i, CG, tiles, H);
        const int c0 = it.cg << 3, w0 = it.tile * DW_TW;
        const int oc0 = (S == 1) ? w0 - 1 : w0 / 2;
        float acc[DW_TW][8];
#pragma unroll
        for (int j = 0; j < DW_TW; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[j][e] = 0.0f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int t = it.row + 1 - kh;
            if (t < 0 || (t % S) != 0) continue;
            const int oh = t / S;
            if (oh >= OH) continue;
            const size_t rowoff = ((it.img * (size_t)OH + (size_t)oh) * (size_t)OW) * (size_t)C + c0;
            uint4 graw[NCOL], yraw[NCOL];
#pragma unroll
            for (int q = 0; q < NCOL; ++q) {
                const int oc = oc0 + q;
                const int occ = min(max(oc, 0), OW - 1);
                graw[q] = *reinterpret_cast<const uint4*>(g + rowoff + (size_t)occ * (size_t)C);
                if (RELU6) yraw[q] = *reinterpret_cast<const uint4*>(y + rowoff + (size_t)occ * (size_t)C);
                if (oc < 0 || oc >= OW) graw[q] = make_uint4(0u, 0u, 0u, 0u);
            }
            Vec8 wk[3];
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) wk[kw] = load_w8(w + (size_t)(kh * 3 + kw) * (size_t)C + c0);
            Vec8 gv[NCOL];
#pragma unroll
            for (int q = 0; q < NCOL; ++q) {
                gv[q] = unpack8(graw[q]);
                if (RELU6) {
                    const Vec8 yv = unpack8(yraw[q]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) gv[q].v[e] = (yv.v[e] > 0.0f && yv.v[e] < 6.0f) ? gv[q].v[e] : 0.0f;
                }
            }
#pragma unroll
            for (int j = 0; j < DW_TW; ++j) {
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    // input column w0 + j gathers through tap kw from output column (w0 + j + 1 - kw) / S; w0 is a
                    // multiple of DW_TW (even), so at stride 2 the parity of d alone decides whether the tap is live
                    const int d = j + 1 - kw;
                    const bool live = (S == 1) || (d >= 0 && d % 2 == 0);
                    if (live) {
                        const int q = (S == 1) ? d + 1 : d / 2;
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[j][e] = fmaf(gv[q].v[e], wk[kw].v[e], acc[j][e]);
                    }
                }
            }
        }
        bf16_t* orow = gx + ((it.img * (size_t)H + (size_t)it.row) * (size_t)W) * (size_t)C + c0;
#pragma unroll
        for (int j = 0; j < DW_TW; ++j) {
            if (w0 + j < W) *reinterpret_cast<uint4*>(orow + (size_t)(w0 + j) * (size_t)C) = pack8(acc[j]);
        }
    }
}

inline bool dw_args_ok(int B, int H, int W, int C, int stride) {
    return B > 0 && H > 0 && W > 0 && C > 0 && (C % 8) == 0 && (stride == 1 || stride == 2);
}

inline unsigned dw_grid(size_t total) {
    const size_t blocks = (total + DW_THREADS - 1) / DW_THREADS;
    return (unsigned)(blocks < ((size_t)1 << 24) ? blocks : ((size_t)1 << 24));     // grid-stride beyond that
}

}  // namespace

extern "C" int adil_dw3x3_fwd(const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int C,
                              int stride, int relu6, void* stream) {
    if (x == nullptr || w == nullptr || y == nullptr || !dw_args_ok(B, H, W, C, stride)) return ADIL_EINVAL;
    if (!aligned(x, 16) || !aligned(w, 16) || !aligned(y, 16) || !aligned(bias, 16)) return ADIL_EINVAL;
    ADIL_ENTER();
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    const size_t total = (size_t)B * (size_t)OH * (size_t)((OW + DW_TW - 1) / DW_TW) * (size_t)(C / 8);
    hipStream_t s = (hipStream_t)stream;
    const bf16_t* xp = (const bf16_t*)x;
    bf16_t* yp = (bf16_t*)y;
    const dim3 grid(dw_grid(total)), block(DW_THREADS);
    if (stride == 1) {
        if (relu6) hipLaunchKernelGGL((dw3x3_fwd_kernel<1, true>), grid, block, 0, s, xp, w, bias, yp, H, W, C, OH, OW, total);
        else hipLaunchKernelGGL((dw3x3_fwd_kernel<1, false>), grid, block, 0, s, xp, w, bias, yp, H, W, C, OH, OW, total);
    } else {
        if (relu6) hipLaunchKernelGGL((dw3x3_fwd_kernel<2, true>), grid, block, 0, s, xp, w, bias, yp, H, W, C, OH, OW, total);
        else hipLaunchKernelGGL((dw3x3_fwd_kernel<2, false>), grid, block, 0, s, xp, w, bias, yp, H, W, C, OH, OW, total);
    }
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_dw3x3_bwd(const void* g, const void* y, const float* w, void* gx, int B, int H, int W, int C,
                              int stride, int relu6, void* stream) {
    if (g == nullptr || w == nullptr || gx == nullptr || (relu6 && y == nullptr) || !dw_args_ok(B, H, W, C, stride))
        return ADIL_EINVAL;
    if (!aligned(g, 16) || !aligned(w, 16) || !aligned(gx, 16) || (relu6 && !aligned(y, 16))) return ADIL_EINVAL;
    ADIL_ENTER();
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    const size_t total = (size_t)B * (size_t)H * (size_t)((W + DW_TW - 1) / DW_TW) * (size_t)(C / 8);
    hipStream_t s = (hipStream_t)stream;
    const bf16_t* gp = (const bf16_t*)g;
    const bf16_t* yp = (const bf16_t*)y;
    bf16_t* op = (bf16_t*)gx;
    const dim3 grid(dw_grid(total)), block(DW_THREADS);
    if (stride == 1) {
        if (relu6) hipLaunchKernelGGL((dw3x3_bwd_kernel<1, true>), grid, block, 0, s, gp, yp, w, op, H, W, C, OH, OW, total);
        else hipLaunchKernelGGL((dw3x3_bwd_kernel<1, false>), grid, block, 0, s, gp, yp, w, op, H, W, C, OH, OW, total);
    } else {
        if (relu6) hipLaunchKernelGGL((dw3x3_bwd_kernel<2, true>), grid, block, 0, s, gp, yp, w, op, H, W, C, OH, OW, total);
        else hipLaunchKernelGGL((dw3x3_bwd_kernel<2, false>), grid, block, 0, s, gp, yp, w, op, H, W, C, OH, OW, total);
    }
    ADIL_CHECK_LAUNCH();
    return 0;
}
