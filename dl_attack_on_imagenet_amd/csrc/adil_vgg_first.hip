// adil_vgg_first.hip — the first group of a frozen VGG11 (Normalize, conv 3 -> 64 3x3 / stride 1 / pad 1 with bias, ReLU,
// MaxPool2d(2, 2)) forward and input gradient, one kernel each way, directly on the attack's own tensors:
// adil_first3x3_pool_fwd / adil_first3x3_pool_bwd (include/adil_hip.h).  x_adv and dLoss/dx_adv are [B][3][H][W] NCHW in the
// stream dtype (fp32 / bf16); the pooled side is [B][H/2][W/2][64] channels_last bf16 with one winner byte per element in
// the format of adil_bias_relu_pool2_*.  H and W even.  The 64-channel tensor at full resolution never reaches memory.
//
// Both kernels are HBM streams (27 MACs per output one way, 576 per input element the other), so the MFMA shapes are
// chosen for simple addressing, as in adil_first_conv.hip.
//   first3x3_pool_fwd  workgroup (4 waves) = 16 x 32 input pixels = 8 x 16 windows of one image.  The 18 x 34 patch is
//                      normalised, rounded to bf16 and staged in LDS as [row][col][4 ch] (channel 3, columns 34 / 35 and
//                      everything outside the image are zeros: the padding of the NORMALISED tensor).  K order per tap
//                      row kh: (kw 0..3, ci 0..3) = 16 values, kw = 3 and ci = 3 carrying zero weights, so a fragment
//                      (8 consecutive k) of pixel (r, c) is 16 bytes at element 4 c + 8 h of patch row r + kh.
//                      mfma_32x32x16: A = weights (rows = 32 output channels, two row blocks), B = patches, and the 32
//                      columns of one instruction are the SAME corner (dh, dw) of 32 windows (2 window rows x 16), so the
//                      four corners of a window meet in one lane's registers and the pool needs no cross-lane step.
//                      Row rho of a block carries channel 16 ((rho >> 2) & 1) + 4 (rho >> 3) + (rho & 3) (+ 32 per
//                      block): a lane's 16 accumulator registers are then 16 CONSECUTIVE channels of one window, stored
//                      as two 16-byte pieces of y and one of idx.  No LDS transpose.
//   first3x3_pool_bwd  workgroup = 16 x 32 input pixels of one image.  The 10 x 18 windows of g and idx that its 18 x 34
//                      halo touches are un-pooled while they are staged: LDS holds gz [18][34][64] bf16 (78 336 bytes, two
//                      workgroups a CU), the 16-byte chunk q of pixel column c at chunk q ^ (c & 7) so that the fragment
//                      reads of 16 neighbouring pixels fall on 16 different bank groups without padding.
//                      mfma_16x16x32: A = weights (rows = ci, 3 of 16 used), B = gz (columns = 16 pixels of a row, K = 32
//                      output channels): two instructions per tap, taps in the order kh * 3 + kw, channels 0..31 before
//                      32..63; 18 instructions per 16 pixels.
// Out-of-range positions are never loaded (predicated, no clamped reads); offsets are 64-bit; no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adil_common.h"
#include "adil_first_patch.h"
#include "adil_hip.h"
#include "adil_mfma.h"

namespace {

#define VF_TH 16                       // input rows of a forward tile
#define VF_TW 32                       // input columns
#define VF_ROWS (VF_TH + 2)            // 18 patch rows
#define VF_USED (VF_TW + 2)            // 34 patch columns carry data; 34 and 35 meet only the zero weights of kw = 3
#define VF_COLS 36                     // staged columns
#define VF_RS (VF_COLS * 4)            // patch row stride (elements): 288 B

template <typename TX>
__global__ __launch_bounds__(256, 3) void first3x3_pool_fwd_kernel(const TX* __restrict__ x, const bf16_t* __restrict__ wf,
                                                                   InputNorm nm, const float* __restrict__ bias,
                                                                   bf16_t* __restrict__ y, unsigned char* __restrict__ idx,
                                                                   int H, int W) {
    __shared__ __attribute__((aligned(16))) bf16_t sin[VF_ROWS * VF_RS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int n = blockIdx.z, ih0 = blockIdx.y * VF_TH, iw0 = blockIdx.x * VF_TW;
    const int OH = H >> 1, OW = W >> 1;
    // input tile: x' = bf16((x - mean) * inv_std), each operation rounded to fp32 on its own; zeros outside the image
    const TX* xn = x + (size_t)n * 3 * (size_t)H * (size_t)W;
    const size_t plane = (size_t)H * (size_t)W;
    constexpr int NPOS = (VF_ROWS * VF_COLS + 255) / 256;
    float raw[NPOS][3];
    bool okm[NPOS];
#pragma unroll
    for (int j = 0; j < NPOS; ++j) {
        const int pos = tid + 256 * j;
        const int row = pos / VF_COLS, col = pos - row * VF_COLS;
        const int ih = ih0 - 1 + row, iw = iw0 - 1 + col;
        okm[j] = (row < VF_ROWS) && (col < VF_USED) && (ih >= 0) && (ih < H) && (iw >= 0) && (iw < W);
        raw[j][0] = raw[j][1] = raw[j][2] = 0.0f;
        if (okm[j]) {
            const size_t at = (size_t)ih * (size_t)W + (size_t)iw;
            raw[j][0] = Elem<TX>::load(xn, at);
            raw[j][1] = Elem<TX>::load(xn + plane, at);
            raw[j][2] = Elem<TX>::load(xn + 2 * plane, at);
        }
    }
    // weights: lane (c, h) holds k = 8h .. 8h+7 of the channel its row carries, for each tap row and row block
    const int chan = 16 * ((c >> 2) & 1) + 4 * (c >> 3) + (c & 3);
    bf16x8 a[2][3];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
            a[blk][kh] = *reinterpret_cast<const bf16x8*>(wf + (blk * 32 + chan) * 48 + kh * 16 + 8 * h);
#pragma unroll
    for (int j = 0; j < NPOS; ++j) {
#pragma clang fp contract(off)
        const int pos = tid + 256 * j;
        const int row = pos / VF_COLS, col = pos - row * VF_COLS;
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
        if (pos < VF_ROWS * VF_COLS) *reinterpret_cast<u32x2*>(sin + row * VF_RS + col * 4) = t;
    }
    lds_sync();
    // wave w: window rows 2w, 2w+1 of the tile; lane c <-> window (2w + c / 16, c % 16)
    const int wr = 2 * w + (c >> 4), wc = c & 15;
    const int oh = (ih0 >> 1) + wr, ow = (iw0 >> 1) + wc;
    bf16x8 b[4][3];                                        // [corner 2 dh + dw][kh]
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            // 8-byte aligned only (odd columns): two 8-byte reads
            const bf16_t* p = sin + (2 * wr + (k >> 1) + kh) * VF_RS + (2 * wc + (k & 1)) * 4 + 8 * h;
            u32x4 t;
            const u32x2 lo = *reinterpret_cast<const u32x2*>(p), hi = *reinterpret_cast<const u32x2*>(p + 4);
            t[0] = lo[0], t[1] = lo[1], t[2] = hi[0], t[3] = hi[1];
            b[k][kh] = __builtin_bit_cast(bf16x8, t);
        }
    }
    const bool live = (oh < OH) && (ow < OW);
    const size_t at = (((size_t)n * (size_t)OH + (size_t)oh) * (size_t)OW + (size_t)ow) * 64;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        f32x16 acc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[k][r] = 0.0f;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) mma16(acc[k], a[blk][kh], b[k][kh]);
        }
        // register r of lane (c, h) = channel co + r of window c, at corner k in acc[k]
        const int co = blk * 32 + 16 * h;
        float bs[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(bias + co + 4 * q);
            bs[4 * q] = t.x, bs[4 * q + 1] = t.y, bs[4 * q + 2] = t.z, bs[4 * q + 3] = t.w;
        }
        float o[16];
        unsigned wi[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float best = acc[0][r] + bs[r];
            unsigned bi = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                const float v = acc[k][r] + bs[r];
                if (v > best) best = v, bi = (unsigned)k;             // the first strictly greater than all before it
            }
            const bool dead = best <= 0.0f;
            o[r] = dead ? 0.0f : best;                                // +0 for a dead window (never -0)
            wi[r] = dead ? 4u : bi;
        }
        if (live) {
            u32x4 y0, y1, iv;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                y0[d] = pack2_bf16(o[2 * d], o[2 * d + 1]);
                y1[d] = pack2_bf16(o[8 + 2 * d], o[8 + 2 * d + 1]);
                iv[d] = wi[4 * d] | (wi[4 * d + 1] << 8) | (wi[4 * d + 2] << 16) | (wi[4 * d + 3] << 24);
            }
            *reinterpret_cast<u32x4*>(y + at + co) = y0;
            *reinterpret_cast<u32x4*>(y + at + co + 8) = y1;
            *reinterpret_cast<u32x4*>(idx + at + co) = iv;
        }
    }
}

// =========================================================================================================== //
// first3x3_pool_bwd:  gx[ci][ih][iw] = inv_std[ci] * sum_{kh,kw,co} gz[ih+1-kh][iw+1-kw][co] * w[co][ci][kh][kw], with
//   gz[h][w][co] = g[h/2][w/2][co] where idx[h/2][w/2][co] == 2 (h & 1) + (w & 1), else +0.
//   v_mfma_f32_16x16x32_bf16: A lane l -> row l&15, k = 8*(l>>4)+j; B lane l -> column l&15, same k; C register r of
//   lane l -> row 4*(l>>4)+r, column l&15.
// =========================================================================================================== //
#define VB_TH 16
#define VB_TW 32
#define VB_HR (VB_TH + 2)              // 18 halo rows of gz
#define VB_HC (VB_TW + 2)              // 34 halo columns
#define VB_PR (VB_TH / 2 + 2)          // 10 window rows of g
#define VB_PC (VB_TW / 2 + 2)          // 18 window columns

typedef float f32x4 __attribute__((ext_vector_type(4)));

// element offset of the 16-byte chunk q (8 channels) of halo pixel (row, col)
__device__ __forceinline__ int vb_at(int row, int col, int q) { return ((row * VB_HC + col) * 8 + (q ^ (col & 7))) * 8; }

template <typename TX>
__global__ __launch_bounds__(256, 2) void first3x3_pool_bwd_kernel(const bf16_t* __restrict__ g,
                                                                   const unsigned char* __restrict__ idx,
                                                                   const bf16_t* __restrict__ wb, InputNorm nm,
                                                                   TX* __restrict__ gx, int H, int W) {
    __shared__ __attribute__((aligned(16))) bf16_t sg[VB_HR * VB_HC * 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l16 = lane & 15, ks = lane >> 4;             // pixel column / K slice of this lane
    const int n = blockIdx.z, ih0 = blockIdx.y * VB_TH, iw0 = blockIdx.x * VB_TW;
    const int OH = H >> 1, OW = W >> 1;
    {   // un-pool 10 x 18 windows x 8 chunks of 8 channels into the 18 x 34 halo: window (i, j) holds halo pixels
        // (2i - 1 + dh, 2j - 1 + dw); every halo pixel is written exactly once, with zeros where its window is off the image
        constexpr int NQ = VB_PR * VB_PC * 8, NGQ = (NQ + 255) / 256;
        const int q = tid & 7;                             // a thread keeps one channel chunk (256 % 8 == 0)
        const int ohb = (ih0 >> 1) - 1, owb = (iw0 >> 1) - 1;
        u32x4 gv[NGQ];
        u32x2 iv[NGQ];
#pragma unroll
        for (int j = 0; j < NGQ; ++j) {
            const int it = tid + 256 * j, px = it >> 3;
            const int i = px / VB_PC, jc = px - i * VB_PC;
            const int oh = ohb + i, ow = owb + jc;
            gv[j] = u32x4{0u, 0u, 0u, 0u};
            iv[j] = u32x2{0u, 0u};
            if ((it < NQ) && (oh >= 0) && (oh < OH) && (ow >= 0) && (ow < OW)) {
                const size_t at = (((size_t)n * (size_t)OH + (size_t)oh) * (size_t)OW + (size_t)ow) * 64 + q * 8;
                gv[j] = *reinterpret_cast<const u32x4*>(g + at);
                iv[j] = *reinterpret_cast<const u32x2*>(idx + at);
            }
        }
#pragma unroll
        for (int j = 0; j < NGQ; ++j) {
            const int it = tid + 256 * j, px = it >> 3;
            const int i = px / VB_PC, jc = px - i * VB_PC;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                u32x4 o;
#pragma unroll
                for (int d = 0; d < 4; ++d) {              // dword d: channels 2d (low half) and 2d + 1 (high half)
                    const unsigned i0 = (iv[j][d >> 1] >> (16 * (d & 1))) & 0xffu, i1 = (iv[j][d >> 1] >> (16 * (d & 1) + 8)) & 0xffu;
                    o[d] = (i0 == (unsigned)k ? (gv[j][d] & 0xffffu) : 0u) | (i1 == (unsigned)k ? (gv[j][d] & 0xffff0000u) : 0u);
                }
                const int row = 2 * i - 1 + (k >> 1), col = 2 * jc - 1 + (k & 1);
                if ((it < NQ) && (row >= 0) && (row < VB_HR) && (col >= 0) && (col < VB_HC))
                    *reinterpret_cast<u32x4*>(sg + vb_at(row, col, q)) = o;
            }
        }
    }
    // weights: rows ci = l16 < 3 of the A operand, one 16-byte read per tap and channel half; the other 13 rows are zeros
    bf16x8 a[9][2];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            a[t][hf] = bf16x8{};
            if (l16 < 3) a[t][hf] = *reinterpret_cast<const bf16x8*>(wb + (l16 * 9 + t) * 64 + 32 * hf + 8 * ks);
        }
    }
    lds_sync();
    // wave w: rows 4w .. 4w+3 of the tile, two groups of 16 columns each
    f32x4 acc[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int cg = 0; cg < 2; ++cg) acc[r][cg] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int cg = 0; cg < 2; ++cg) {
                    const int row = 4 * w + r + 2 - kh, col = 16 * cg + l16 + 2 - kw;      // halo pixel of (ih + 1 - kh, iw + 1 - kw)
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
                        const bf16x8 b = lds8(sg + vb_at(row, col, 4 * hf + ks));
                        acc[r][cg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kh * 3 + kw][hf], b, acc[r][cg], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (ks == 0) {                                         // accumulator rows 0..2 (= ci) are registers 0..2 of lanes 0..15
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int cg = 0; cg < 2; ++cg) {
                const int ih = ih0 + 4 * w + r, iw = iw0 + 16 * cg + l16;
                if (ih < H && iw < W) {
#pragma unroll
                    for (int ci = 0; ci < 3; ++ci) {
                        const size_t at = (((size_t)n * 3 + ci) * (size_t)H + (size_t)ih) * (size_t)W + (size_t)iw;
                        Elem<TX>::store(gx, at, acc[r][cg][ci] * nm.inv_std[ci]);
                    }
                }
            }
        }
    }
}

// the shared argument check; the image index and the tile row are grid dimensions
inline bool vgg_first_args_ok(int B, int H, int W, int dtype) {
    if (B <= 0 || B > 65535 || H < 2 || W < 2 || (H & 1) || (W & 1)) return false;
    if ((long long)B * H * W > 0x7fffffffLL) return false;
    if ((H + VF_TH - 1) / VF_TH > 65535) return false;
    return dtype == ADIL_F32 || dtype == ADIL_BF16;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------ //
extern "C" int adil_first3x3_pool_fwd(const void* x, int x_dtype, const void* w_fwd, float mean0, float mean1, float mean2,
                                      float inv_std0, float inv_std1, float inv_std2, const float* bias, void* y, void* idx,
                                      int B, int H, int W, void* stream) {
    if (!x || !w_fwd || !bias || !y || !idx || !vgg_first_args_ok(B, H, W, x_dtype)) return ADIL_EINVAL;
    if (!aligned(x, x_dtype == ADIL_F32 ? 4 : 2) || !aligned(w_fwd, 16) || !aligned(bias, 16) || !aligned(y, 16) ||
        !aligned(idx, 16))
        return ADIL_EINVAL;
    ADIL_ENTER();
    const InputNorm nm = {{mean0, mean1, mean2}, {inv_std0, inv_std1, inv_std2}};
    const dim3 grid((W + VF_TW - 1) / VF_TW, (H + VF_TH - 1) / VF_TH, B), block(256);
    hipStream_t st = (hipStream_t)stream;
    const bf16_t* wp = (const bf16_t*)w_fwd;
    if (x_dtype == ADIL_F32)
        hipLaunchKernelGGL((first3x3_pool_fwd_kernel<float>), grid, block, 0, st, (const float*)x, wp, nm, bias, (bf16_t*)y,
                           (unsigned char*)idx, H, W);
    else
        hipLaunchKernelGGL((first3x3_pool_fwd_kernel<bf16_t>), grid, block, 0, st, (const bf16_t*)x, wp, nm, bias, (bf16_t*)y,
                           (unsigned char*)idx, H, W);
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_first3x3_pool_bwd(const void* g, const void* idx, const void* w_bwd, float inv_std0, float inv_std1,
                                      float inv_std2, void* gx, int gx_dtype, int B, int H, int W, void* stream) {
    if (!g || !idx || !w_bwd || !gx || !vgg_first_args_ok(B, H, W, gx_dtype)) return ADIL_EINVAL;
    if (!aligned(g, 16) || !aligned(idx, 8) || !aligned(w_bwd, 16) || !aligned(gx, gx_dtype == ADIL_F32 ? 4 : 2))
        return ADIL_EINVAL;
    ADIL_ENTER();
    const InputNorm nm = {{0.0f, 0.0f, 0.0f}, {inv_std0, inv_std1, inv_std2}};
    const dim3 grid((W + VB_TW - 1) / VB_TW, (H + VB_TH - 1) / VB_TH, B), block(256);
    hipStream_t st = (hipStream_t)stream;
    const bf16_t* gp = (const bf16_t*)g;
    const unsigned char* ip = (const unsigned char*)idx;
    const bf16_t* wp = (const bf16_t*)w_bwd;
    if (gx_dtype == ADIL_F32)
        hipLaunchKernelGGL((first3x3_pool_bwd_kernel<float>), grid, block, 0, st, gp, ip, wp, nm, (float*)gx, H, W);
    else
        hipLaunchKernelGGL((first3x3_pool_bwd_kernel<bf16_t>), grid, block, 0, st, gp, ip, wp, nm, (bf16_t*)gx, H, W);
    ADIL_CHECK_LAUNCH();
    return 0;
}
