// adil_first_conv.hip — the first convolution of the frozen MobileNetV2 (3 -> 32, 3x3, stride 2, pad 1) with the
// Normalize in front of it and its eval-BatchNorm + ReLU6 behind it, forward and input gradient, directly on the attack's
// own tensors: adil_first3x3_fwd / adil_first3x3_bwd (include/adil_hip.h).  x_adv and dLoss/dx_adv are [B][3][H][W] NCHW
// in the stream dtype (fp32 / bf16), the activation side is [B][OH][OW][32] channels_last bf16.  Any H, W >= 1.
//
// Both kernels follow the ResNet stem's (adil_stem.hip) and are HBM streams: 864 MACs per output pixel is nothing for
// the matrix pipe, so the MFMA shapes are chosen for simple addressing, not for K efficiency.
//   first3x3_fwd   workgroup (4 waves) = 16 x 16 outputs of one image.  The 33 x 33 input patch is normalised, rounded
//                  to bf16 and staged in LDS as [row][col][4 ch] (channel 3 and everything outside the image are zeros:
//                  the padding of the NORMALISED tensor).  K order per tap row kh: (kw 0..3, ci 0..3) = 16 values, kw = 3
//                  and ci = 3 carrying zero weights, so a fragment (8 consecutive k) of output pixel (oh, ow) is one
//                  aligned 16-byte LDS read at element 8 ow + 8 h of row 2 oh + kh: three mfma_32x32x16 per 32 pixels.
//                  A = weights (rows = the 32 output channels, read straight from global memory: 3 x 16 bytes a lane),
//                  B = patches (columns = pixels); a per-wave LDS transpose gives 16-byte channels_last stores.
//   first3x3_bwd   workgroup = 16 x 32 input pixels of one image = 4 parity classes x (8 x 16) pixels with 1 / 2 / 2 / 4
//                  live taps.  gz = bf16(g * scale) [0 < y < 6] is formed while the 9 x 17 tile of g is staged in LDS.
//                  mfma_16x16x32: A = weights (rows = ci, 3 of 16 used), B = gz (columns = pixels, K = the 32 output
//                  channels: one instruction per tap), 18 instructions per wave.  g is never zero-upsampled.
// Out-of-range positions are never loaded (predicated, no clamped reads); offsets are 64-bit; no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adil_common.h"
#include "adil_first_patch.h"
#include "adil_hip.h"
#include "adil_mfma.h"

namespace {

#define FC_T 16                        // conv-output tile edge
#define FC_ROWS (2 * FC_T + 1)         // 33 input rows
#define FC_USED (2 * FC_T + 1)         // 33 input columns carry data; column 33 meets only the zero weights of kw = 3
#define FC_COLS 36                     // staged columns (33 .. 35 are zeros)
#define FC_RS (FC_COLS * 4 + 8)        // input row stride (elements): 304 B = 19 x 16 B
#define FC_OS 40                       // staged-output pixel stride (elements): 80 B = 5 x 16 B

template <typename TX, bool RELU6>
__global__ __launch_bounds__(256) void first3x3_fwd_kernel(const TX* __restrict__ x, const bf16_t* __restrict__ wf,
                                                           InputNorm nm, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, bf16_t* __restrict__ y,
                                                           int H, int W, int OH, int OW) {
    __shared__ __attribute__((aligned(16))) bf16_t sin[FC_ROWS * FC_RS];
    __shared__ __attribute__((aligned(16))) bf16_t sout[4 * 32 * FC_OS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int n = blockIdx.z, oh0 = blockIdx.y * FC_T, ow0 = blockIdx.x * FC_T;
    // weights: lane (c, h) holds k = 8h .. 8h+7 of output channel c for each tap row
    bf16x8 a[3];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) a[kh] = *reinterpret_cast<const bf16x8*>(wf + c * 48 + kh * 16 + 8 * h);
    // input tile: x' = bf16((x - mean) * inv_std), each operation rounded to fp32 on its own; zeros outside the image
    const TX* xn = x + (size_t)n * 3 * (size_t)H * (size_t)W;
    const size_t plane = (size_t)H * (size_t)W;
    constexpr int NPOS = (FC_ROWS * FC_COLS + 255) / 256;
    float raw[NPOS][3];
    bool okm[NPOS];
#pragma unroll
    for (int j = 0; j < NPOS; ++j) {
        const int pos = tid + 256 * j;
        const int row = pos / FC_COLS, col = pos - row * FC_COLS;
        const int ih = 2 * oh0 - 1 + row, iw = 2 * ow0 - 1 + col;
        okm[j] = (row < FC_ROWS) && (col < FC_USED) && (ih >= 0) && (ih < H) && (iw >= 0) && (iw < W);
        raw[j][0] = raw[j][1] = raw[j][2] = 0.0f;
        if (okm[j]) {
            const size_t at = (size_t)ih * (size_t)W + (size_t)iw;
            raw[j][0] = Elem<TX>::load(xn, at);
            raw[j][1] = Elem<TX>::load(xn + plane, at);
            raw[j][2] = Elem<TX>::load(xn + 2 * plane, at);
        }
    }
#pragma unroll
    for (int j = 0; j < NPOS; ++j) {
#pragma clang fp contract(off)
        const int pos = tid + 256 * j;
        const int row = pos / FC_COLS, col = pos - row * FC_COLS;
        float v[3];
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
            const float d = raw[j][ci] - nm.mean[ci];
            const float p = d * nm.inv_std[ci];
            v[ci] = okm[j] ? p : 0.0f;
        }
        u32x2 t;
        t[0] = pack2_bf16(v[0], v[1]);
        t[1] = pack2_bf16(v[2], 0.0f);
        if (pos < FC_ROWS * FC_COLS) *reinterpret_cast<u32x2*>(sin + row * FC_RS + col * 4) = t;
    }
    lds_sync();
    // wave w: pixel tiles 2w, 2w+1 (tile t = conv rows 2t, 2t+1 x 16 columns; lane c <-> (c / 16, c % 16))
    f32x16 acc[2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[p][r] = 0.0f;
    const int prow = c >> 4, pcol = c & 15;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int orow = 2 * (2 * w + p) + prow;
            const bf16x8 b = lds8(sin + (2 * orow + kh) * FC_RS + 8 * pcol + 8 * h);
            mma16(acc[p], a[kh], b);
        }
    }
    // epilogue: BN affine + ReLU6 (every pre-activation <= 0 becomes +0), per-wave transpose through LDS, 16-byte stores
    bf16_t* so = sout + w * 32 * FC_OS;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int co = 8 * q + 4 * h;                  // accumulator register 4q + j of lane (c, h) = channel co + j
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float z = acc[p][4 * q + j] * scale[co + j] + shift[co + j];
                if (RELU6) v[j] = (z <= 0.0f) ? 0.0f : fminf(z, 6.0f);
                else v[j] = (z == 0.0f) ? 0.0f : z;
            }
            u32x2 t;
            t[0] = pack2_bf16(v[0], v[1]);
            t[1] = pack2_bf16(v[2], v[3]);
            *reinterpret_cast<u32x2*>(so + c * FC_OS + co) = t;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = lane + 64 * i, px = id >> 2, ch = (id & 3) * 8;
            const int oh = oh0 + 2 * (2 * w + p) + (px >> 4), ow = ow0 + (px & 15);
            const u32x4 t = *reinterpret_cast<const u32x4*>(so + px * FC_OS + ch);
            if (oh < OH && ow < OW)
                *reinterpret_cast<u32x4*>(y + (((size_t)n * (size_t)OH + (size_t)oh) * (size_t)OW + (size_t)ow) * 32 + ch) = t;
        }
    }
}

// =========================================================================================================== //
// first3x3_bwd:  gx[ci][ih][iw] = inv_std[ci] * sum_{kh,kw,co} gz[(ih+1-kh)/2][(iw+1-kw)/2][co] * w[co][ci][kh][kw]
//   over the taps with even ih+1-kh, iw+1-kw.  Parity class (A, BB) = (ih & 1, iw & 1): taps kh = 1 - A, 3 - A, ... < 3.
//   Wave w takes block rows 2w, 2w+1 (a block = 2 x 2 input pixels) of every class; lane l16 = block column.
//   v_mfma_f32_16x16x32_bf16: A lane l -> row l&15, k = 8*(l>>4)+j; B lane l -> column l&15, same k; C register r of
//   lane l -> row 4*(l>>4)+r, column l&15.
// =========================================================================================================== //
#define FB_TH 16
#define FB_TW 32
#define FB_GR (FB_TH / 2 + 1)          // 9 rows of g
#define FB_GC (FB_TW / 2 + 1)          // 17 columns of g
#define FB_PS 40                       // gz pixel stride in LDS (elements): 80 B = 5 x 16 B

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int A, int BB>
__device__ __forceinline__ void first_bwd_class(f32x4 (&acc)[2], const bf16_t* sg, const bf16x8 (&a)[9], int w, int l16,
                                                int ks) {
#pragma unroll
    for (int kh = 1 - A; kh < 3; kh += 2) {
#pragma unroll
        for (int kw = 1 - BB; kw < 3; kw += 2) {
            const int col = l16 + (BB + 1 - kw) / 2;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int row = 2 * w + q + (A + 1 - kh) / 2;
                const bf16x8 b = lds8(sg + (row * FB_GC + col) * FB_PS + 8 * ks);
                acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kh * 3 + kw], b, acc[q], 0, 0, 0);
            }
        }
    }
}

template <typename TX, bool RELU6>
__global__ __launch_bounds__(256) void first3x3_bwd_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ y,
                                                           const float* __restrict__ scale, const bf16_t* __restrict__ wb,
                                                           InputNorm nm, TX* __restrict__ gx, int H, int W, int OH,
                                                           int OW) {
    __shared__ __attribute__((aligned(16))) bf16_t sg[FB_GR * FB_GC * FB_PS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l16 = lane & 15, ks = lane >> 4;             // block column / K slice of this lane
    const int n = blockIdx.z, ih0 = blockIdx.y * FB_TH, iw0 = blockIdx.x * FB_TW;
    // weights: rows ci = l16 < 3 of the A operand, one 16-byte read per tap; the other 13 rows are zeros
    bf16x8 a[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        a[t] = bf16x8{};
        if (l16 < 3) a[t] = *reinterpret_cast<const bf16x8*>(wb + (l16 * 9 + t) * 32 + 8 * ks);
    }
    {   // gz tile: 9 x 17 pixels x 4 chunks of 8 channels; a thread keeps one channel chunk (256 % 4 == 0)
        constexpr int NQ = FB_GR * FB_GC * 4, NGQ = (NQ + 255) / 256;
        const int ch = tid & 3;
        float sc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) sc[e] = scale[ch * 8 + e];
        const int ohb = ih0 / 2, owb = iw0 / 2;
        u32x4 gv[NGQ], yv[NGQ];
        bool ok[NGQ];
#pragma unroll
        for (int j = 0; j < NGQ; ++j) {
            const int q = tid + 256 * j, px = q >> 2;
            const int row = px / FB_GC, col = px - row * FB_GC;
            const int oh = ohb + row, ow = owb + col;
            ok[j] = (q < NQ) && (oh < OH) && (ow < OW);
            gv[j] = u32x4{0u, 0u, 0u, 0u};
            yv[j] = u32x4{0u, 0u, 0u, 0u};
            if (ok[j]) {
                const size_t at = (((size_t)n * (size_t)OH + (size_t)oh) * (size_t)OW + (size_t)ow) * 32 + ch * 8;
                gv[j] = *reinterpret_cast<const u32x4*>(g + at);
                if (RELU6) yv[j] = *reinterpret_cast<const u32x4*>(y + at);
            }
        }
#pragma unroll
        for (int j = 0; j < NGQ; ++j) {
            const int q = tid + 256 * j, px = q >> 2;
            float gf[8], yf[8];
            unpack8(gv[j], gf);
            unpack8(yv[j], yf);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = gf[e] * sc[e];
                if (RELU6) v = (yf[e] > 0.0f && yf[e] < 6.0f) ? v : 0.0f;
                gf[e] = ok[j] ? v : 0.0f;
            }
            if (q < NQ) *reinterpret_cast<u32x4*>(sg + px * FB_PS + ch * 8) = pack8(gf);
        }
    }
    lds_sync();
    f32x4 acc[4][2];                                       // [parity class][block row 2w + q]
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[k][q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    first_bwd_class<0, 0>(acc[0], sg, a, w, l16, ks);
    first_bwd_class<0, 1>(acc[1], sg, a, w, l16, ks);
    first_bwd_class<1, 0>(acc[2], sg, a, w, l16, ks);
    first_bwd_class<1, 1>(acc[3], sg, a, w, l16, ks);
    if (ks == 0) {                                         // accumulator rows 0..2 (= ci) are registers 0..2 of lanes 0..15
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ih = ih0 + 2 * (2 * w + q) + (k >> 1), iw = iw0 + 2 * l16 + (k & 1);
                if (ih < H && iw < W) {
#pragma unroll
                    for (int ci = 0; ci < 3; ++ci) {
                        const size_t at = (((size_t)n * 3 + ci) * (size_t)H + (size_t)ih) * (size_t)W + (size_t)iw;
                        Elem<TX>::store(gx, at, acc[k][q][ci] * nm.inv_std[ci]);
                    }
                }
            }
        }
    }
}

inline bool first_args_ok(int B, int H, int W, int dtype, int relu6) {
    // gridDim.z carries the image index
    return B > 0 && B <= 65535 && H > 0 && W > 0 && (dtype == ADIL_F32 || dtype == ADIL_BF16) && (relu6 == 0 || relu6 == 1);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------ //
extern "C" int adil_first3x3_fwd(const void* x, int x_dtype, const void* w_fwd, float mean0, float mean1, float mean2,
                                 float inv_std0, float inv_std1, float inv_std2, const float* scale, const float* shift,
                                 void* y, int B, int H, int W, int relu6, void* stream) {
    if (!x || !w_fwd || !scale || !shift || !y || !first_args_ok(B, H, W, x_dtype, relu6)) return ADIL_EINVAL;
    if (!aligned(x, x_dtype == ADIL_F32 ? 4 : 2) || !aligned(w_fwd, 16) || !aligned(y, 16) || !aligned(scale, 4) ||
        !aligned(shift, 4))
        return ADIL_EINVAL;
    ADIL_ENTER();
    const InputNorm nm = {{mean0, mean1, mean2}, {inv_std0, inv_std1, inv_std2}};
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const dim3 grid((OW + FC_T - 1) / FC_T, (OH + FC_T - 1) / FC_T, B), block(256);
    if (grid.y > 65535u) return ADIL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const bf16_t* wp = (const bf16_t*)w_fwd;
    bf16_t* yp = (bf16_t*)y;
    if (x_dtype == ADIL_F32) {
        if (relu6) hipLaunchKernelGGL((first3x3_fwd_kernel<float, true>), grid, block, 0, st, (const float*)x, wp, nm, scale, shift, yp, H, W, OH, OW);
        else hipLaunchKernelGGL((first3x3_fwd_kernel<float, false>), grid, block, 0, st, (const float*)x, wp, nm, scale, shift, yp, H, W, OH, OW);
    } else {
        if (relu6) hipLaunchKernelGGL((first3x3_fwd_kernel<bf16_t, true>), grid, block, 0, st, (const bf16_t*)x, wp, nm, scale, shift, yp, H, W, OH, OW);
        else hipLaunchKernelGGL((first3x3_fwd_kernel<bf16_t, false>), grid, block, 0, st, (const bf16_t*)x, wp, nm, scale, shift, yp, H, W, OH, OW);
    }
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_first3x3_bwd(const void* g, const void* y, const float* scale, const void* w_bwd, float inv_std0,
                                 float inv_std1, float inv_std2, void* gx, int gx_dtype, int B, int H, int W, int relu6,
                                 void* stream) {
    if (!g || !scale || !w_bwd || !gx || !first_args_ok(B, H, W, gx_dtype, relu6) || (relu6 && !y)) return ADIL_EINVAL;
    if (!aligned(g, 16) || !aligned(w_bwd, 16) || (relu6 && !aligned(y, 16)) || !aligned(scale, 4) ||
        !aligned(gx, gx_dtype == ADIL_F32 ? 4 : 2))
        return ADIL_EINVAL;
    ADIL_ENTER();
    const InputNorm nm = {{0.0f, 0.0f, 0.0f}, {inv_std0, inv_std1, inv_std2}};
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const dim3 grid((W + FB_TW - 1) / FB_TW, (H + FB_TH - 1) / FB_TH, B), block(256);
    if (grid.y > 65535u) return ADIL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const bf16_t* gp = (const bf16_t*)g;
    const bf16_t* yp = (const bf16_t*)y;
    const bf16_t* wp = (const bf16_t*)w_bwd;
    if (gx_dtype == ADIL_F32) {
        if (relu6) hipLaunchKernelGGL((first3x3_bwd_kernel<float, true>), grid, block, 0, st, gp, yp, scale, wp, nm, (float*)gx, H, W, OH, OW);
        else hipLaunchKernelGGL((first3x3_bwd_kernel<float, false>), grid, block, 0, st, gp, yp, scale, wp, nm, (float*)gx, H, W, OH, OW);
    } else {
        if (relu6) hipLaunchKernelGGL((first3x3_bwd_kernel<bf16_t, true>), grid, block, 0, st, gp, yp, scale, wp, nm, (bf16_t*)gx, H, W, OH, OW);
        else hipLaunchKernelGGL((first3x3_bwd_kernel<bf16_t, false>), grid, block, 0, st, gp, yp, scale, wp, nm, (bf16_t*)gx, H, W, OH, OW);
    }
    ADIL_CHECK_LAUNCH();
    return 0;
}
