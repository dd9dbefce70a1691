// adil_stem.hip — the frozen classifier's ResNet stem, either side of the ADiL hot path (gfx950).
//
// The attack hands x_adv = x + D v (NCHW, bf16/fp32) to the classifier and takes dLoss/dx_adv back.  For the
// torchvision ResNets the reference attacks (demo_dL_attack.py:41-59) the first stage
//     Normalize -> conv 7x7/2 (3 -> 64) -> BatchNorm(eval) -> ReLU -> maxpool 3x3/2
// is where a library convolution is weakest: 3 input channels (MIOpen pads / transposes in and out, zero-fills,
// 1.4 ms forward and 4.4 ms input gradient at B = 512) and a 9-read pooling kernel.  These kernels do the stage
// directly on the attack's own tensor layouts:
//   stem_conv_fwd   x_adv (NCHW)  -> y1 (NHWC bf16) = relu(bn(conv(normalize(x))))     implicit GEMM on MFMA
//   maxpool_fwd     y1 -> p (NHWC), argmax index (1 byte / element)
//   stem_pool_bwd   g_p, idx, p -> g_y1 = route(g_p) * [p > 0] * bn_scale             (maxpool + ReLU + BN backward)
//   stem_conv_bwd   g_y1 -> g_x (NCHW, the layout adil_grad consumes)                  implicit GEMM on MFMA
// Not part of the ADiL maths: the parity target is the plain PyTorch stem (tests/test_gpu_stem.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adil_common.h"
#include "adil_first_patch.h"                          // InputNorm
#include "adil_hip.h"
#include "adil_mfma.h"

namespace {

// =========================================================================================================== //
// stem_conv_fwd.  Workgroup (4 waves) = a 16 x 16 tile of conv outputs of one image, all 64 channels.
//   K order per tap row kh: (kw 0..7, ci 0..3) = 32 values, kw = 7 and ci = 3 carrying zero weights, so that with the
//   input tile staged in LDS as [row][col][4 ch] a fragment (8 consecutive k) of output pixel (oh, ow) is ONE aligned
//   16-byte read at element 8*ow + 16*g + 8*h of row 2*oh + kh.  K = 7 * 32 = 224 (14 k-groups of 16).
//   MFMA roles: A = weights (rows = output channels), B = patches (columns = pixels), so a lane ends up with 4
//   consecutive channels of ONE pixel per register quad; a per-wave LDS transpose then gives 16-byte NHWC stores.
// =========================================================================================================== //
#define ST_T 16                        // conv-output tile edge
#define ST_ROWS (2 * ST_T + 5)         // 37 input rows
#define ST_COLS 40                     // 38 input columns used (kw = 7 pad reaches column 2*15 + 7), padded
#define ST_RS (ST_COLS * 4 + 8)        // input row stride (elements): 336 B = 21 x 16 B
#define ST_K 224
#define ST_WS (ST_K + 8)               // weight row stride (elements): 464 B = 29 x 16 B
#define ST_OS 72                       // staged-output pixel stride (elements)

template <typename TX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void stem_conv_fwd_kernel(const TX* __restrict__ x, const bf16_t* __restrict__ wf,
                                                            InputNorm nm, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, bf16_t* __restrict__ y,
                                                            int H, int W, int OH, int OW) {
    // one LDS block: [input tile | weights]; the per-wave output-transpose scratch aliases it once the MFMAs are done
    // (42 KB instead of 60 KB: 3 workgroups per CU)
    __shared__ __attribute__((aligned(16))) bf16_t smem[ST_ROWS * ST_RS + 64 * ST_WS];
    static_assert(4 * 32 * ST_OS <= ST_ROWS * ST_RS + 64 * ST_WS, "output scratch must fit in the tile buffers");
    bf16_t* sin = smem;
    bf16_t* sw = smem + ST_ROWS * ST_RS;
    bf16_t* sout = smem;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int n = blockIdx.z, oh0 = blockIdx.y * ST_T, ow0 = blockIdx.x * ST_T;
    // weights: 64 rows x 224 bf16 = 28 chunks of 16 B per row
    {
        u32x4 wv[7];                                       // 64 * 28 = 7 * 256 chunks: all in flight together
#pragma unroll
        for (int j = 0; j < 7; ++j) wv[j] = *reinterpret_cast<const u32x4*>(wf + (size_t)(tid + 256 * j) * 8);
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int q = tid + 256 * j, co = q / 28, off = q - co * 28;
            *reinterpret_cast<u32x4*>(sw + co * ST_WS + off * 8) = wv[j];
        }
    }
    // input tile, normalised, zero outside the image (the padding of the normalised tensor), 4th channel zero
    const TX* xn = x + (size_t)n * 3 * H * W;
    // (all 18 loads of a thread are issued before the first conversion: a rolled loop pays one memory round trip per
    // position)
    constexpr int NPOS = (ST_ROWS * ST_COLS + 255) / 256;
    float raw[NPOS][3], okm[NPOS];
#pragma unroll
    for (int j = 0; j < NPOS; ++j) {
        const int pos = tid + 256 * j < ST_ROWS * ST_COLS ? tid + 256 * j : ST_ROWS * ST_COLS - 1;
        const int row = pos / ST_COLS, col = pos - row * ST_COLS;
        const int ih = 2 * oh0 - 3 + row, iw = 2 * ow0 - 3 + col;
        const bool ok = (ih >= 0) && (ih < H) && (iw >= 0) && (iw < W);
        const size_t at = (size_t)(ok ? ih : 0) * W + (ok ? iw : 0);
        okm[j] = ok ? 1.0f : 0.0f;
        raw[j][0] = Elem<TX>::load(xn, at);
        raw[j][1] = Elem<TX>::load(xn + (size_t)H * W, at);
        raw[j][2] = Elem<TX>::load(xn + (size_t)2 * H * W, at);
    }
#pragma unroll
    for (int j = 0; j < NPOS; ++j) {
        const int pos = tid + 256 * j;
        const int row = pos / ST_COLS, col = pos - row * ST_COLS;
        const float v0 = (raw[j][0] - nm.mean[0]) * nm.inv_std[0] * okm[j];
        const float v1 = (raw[j][1] - nm.mean[1]) * nm.inv_std[1] * okm[j];
        const float v2 = (raw[j][2] - nm.mean[2]) * nm.inv_std[2] * okm[j];
        u32x2 t;
        t[0] = pack2_bf16(v0, v1);
        t[1] = pack2_bf16(v2, 0.0f);
        if (pos < ST_ROWS * ST_COLS) *reinterpret_cast<u32x2*>(sin + row * ST_RS + col * 4) = t;
    }
    lds_sync();
    // wave w: pixel tiles 2w, 2w+1 (tile t = conv rows 2t, 2t+1 x 16 columns; lane c <-> (c / 16, c % 16))
    f32x16 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[p][ct][r] = 0.0f;
    const int prow = c >> 4, pcol = c & 15;
#pragma unroll 1
    for (int kh = 0; kh < 7; ++kh) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            bf16x8 a[2], b[2];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) a[ct] = lds8(sw + (ct * 32 + c) * ST_WS + kh * 32 + 16 * g + 8 * h);
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int orow = 2 * (2 * w + p) + prow;
                b[p] = lds8(sin + (2 * orow + kh) * ST_RS + 8 * pcol + 16 * g + 8 * h);
            }
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) mma16(acc[p][ct], a[ct], b[p]);
        }
    }
    // epilogue: BN affine + ReLU, per-wave transpose through LDS, 16-byte NHWC stores
    lds_sync();                                            // every wave is done reading the tiles the scratch aliases
    bf16_t* so = sout + w * 32 * ST_OS;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co = ct * 32 + 8 * q + 4 * h;
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = fmaxf(acc[p][ct][4 * q + j] * scale[co + j] + shift[co + j], 0.0f);
                u32x2 t;
                t[0] = pack2_bf16(v[0], v[1]);
                t[1] = pack2_bf16(v[2], v[3]);
                *reinterpret_cast<u32x2*>(so + c * ST_OS + co) = t;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int id = lane + 64 * i, px = id >> 3, ch = (id & 7) * 8;
            const int oh = oh0 + 2 * (2 * w + p) + (px >> 4), ow = ow0 + (px & 15);
            const u32x4 t = *reinterpret_cast<const u32x4*>(so + px * ST_OS + ch);
            if (oh < OH && ow < OW) *reinterpret_cast<u32x4*>(y + (((size_t)n * OH + oh) * OW + ow) * 64 + ch) = t;
        }
    }
}

// =========================================================================================================== //
// maxpool 3x3 / stride 2 / pad 1 on NHWC bf16, 8 channels per thread; also records the argmax position
// (kh * 3 + kw, first maximum in scan order under >, a NaN always replaces the running value so the LAST NaN of a window
// wins — the rule of torch's max_pool2d) for the backward.  Padding taps are skipped, not read as zeros.
// =========================================================================================================== //

__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const bf16_t* __restrict__ y, bf16_t* __restrict__ p,
                                                          uint8_t* __restrict__ idx, int B, int OH, int OW, int PH, int PW,
                                                          int C8) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)B * PH * PW * C8;
    if (i >= total) return;
    const int c8 = (int)(i % C8);
    size_t r = i / C8;
    const int pw = (int)(r % PW); r /= PW;
    const int ph = (int)(r % PH);
    const int n = (int)(r / PH);
    float best[8];
    unsigned bi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; bi[j] = 0xffu; }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int oh = 2 * ph - 1 + kh;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int ow = 2 * pw - 1 + kw;
            if (oh >= 0 && oh < OH && ow >= 0 && ow < OW) {
                const u32x4 t = *reinterpret_cast<const u32x4*>(y + ((((size_t)n * OH + oh) * OW + ow) * C8 + c8) * 8);
                float f[8];
                unpack8(t, f);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool take = (f[j] > best[j]) || (f[j] != f[j]) || (bi[j] == 0xffu);
                    best[j] = take ? f[j] : best[j];
                    bi[j] = take ? (unsigned)(kh * 3 + kw) : bi[j];
                }
            }
        }
    }
    *reinterpret_cast<u32x4*>(p + i * 8) = pack8(best);
    u32x2 o;
    o[0] = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
    o[1] = bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24);
    *reinterpret_cast<u32x2*>(idx + i * 8) = o;
}

// =========================================================================================================== //
// stem_pool_bwd, quad form: maxpool backward fused with the ReLU mask (the routed element equals the pooled value p, so
// [y1 > 0] == [p > 0]: y1 itself is not needed) and the eval-BatchNorm scale.  g_y1 is the gradient wrt the convolution
// output; a conv-output pixel sums the gradients of the <= 4 windows that contain it and name it as their argmax.
// The pooled grid is also the grid of 2 x 2 quads of conv-output pixels (PH = ceil(OH / 2), PW = ceil(OW / 2)): one
// thread per (n, a, b, 8 channels) loads the four windows (a, b), (a, b+1), (a+1, b), (a+1, b+1) up front — idx, g and
// p each, clamped and masked at the far edges, 12 loads in flight — and writes the up to four pixels (2a + {0,1},
// 2b + {0,1}).  Per element the sum runs over window rows, then window columns; a masked window adds +0 to a sum that
// is never -0, which changes no bit.  A pooled element is fetched by 4 threads, not 9; n and a come from blockIdx (no
// 64-bit division).
// =========================================================================================================== //
__global__ __launch_bounds__(256) void stem_pool_bwd_quad_kernel(const bf16_t* __restrict__ g, const uint8_t* __restrict__ idx,
                                                                 const bf16_t* __restrict__ p, const float* __restrict__ scale,
                                                                 bf16_t* __restrict__ gy, int OH, int OW, int PH, int PW,
                                                                 int C8) {
    const unsigned j = blockIdx.y * 256u + threadIdx.x;    // (b, c8) of this row of quads
    if (j >= (unsigned)PW * (unsigned)C8) return;
    const int b = (int)(j / (unsigned)C8), c8 = (int)(j - (unsigned)b * (unsigned)C8);
    const int n = (int)(blockIdx.x / (unsigned)PH), a = (int)(blockIdx.x - (unsigned)n * (unsigned)PH);
    const bool oka = a + 1 < PH, okb = b + 1 < PW;
    const int a1 = oka ? a + 1 : a, b1 = okb ? b + 1 : b;
    const size_t r0 = ((size_t)n * PH + a) * PW, r1 = ((size_t)n * PH + a1) * PW;
    const size_t at[4] = {((r0 + b) * C8 + c8) * 8, ((r0 + b1) * C8 + c8) * 8, ((r1 + b) * C8 + c8) * 8,
                          ((r1 + b1) * C8 + c8) * 8};
    u32x2 id[4];
    u32x4 gt[4], pt[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        id[k] = *reinterpret_cast<const u32x2*>(idx + at[k]);
        gt[k] = *reinterpret_cast<const u32x4*>(g + at[k]);
        pt[k] = *reinterpret_cast<const u32x4*>(p + at[k]);
    }
    const bool okw[4] = {true, okb, oka, oka && okb};
    float sc[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) sc[jj] = scale[c8 * 8 + jj];
    // routed[k][jj]: the gradient of window k where its argmax byte and ReLU sign admit it; the argmax byte is tested
    // per pixel below (a window reaches up to 4 of the quad's pixels under different bytes)
    float gf[4][8];
    bool pos[4][8];
    unsigned kk[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float pf[8];
        unpack8(gt[k], gf[k]);
        unpack8(pt[k], pf);
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            kk[k][jj] = (id[k][jj >> 2] >> (8 * (jj & 3))) & 0xffu;
            pos[k][jj] = okw[k] && pf[jj] > 0.0f;
        }
    }
    // pixel (2a + dy, 2b + dx): windows by row, then column, want = kh * 3 + kw of the pixel inside window k
    //   (0,0): k0 @ 4          (0,1): k0 @ 5, k1 @ 3          (1,0): k0 @ 7, k2 @ 1          (1,1): k0 @ 8, k1 @ 6, k2 @ 2, k3 @ 0
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int oh = 2 * a + dy, ow = 2 * b + dx;
            float acc[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) acc[jj] = 0.0f;
#pragma unroll
            for (int wy = 0; wy <= dy; ++wy) {
#pragma unroll
                for (int wx = 0; wx <= dx; ++wx) {
                    const int k = 2 * wy + wx;
                    const unsigned want = (unsigned)((dy + 1 - 2 * wy) * 3 + (dx + 1 - 2 * wx));
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) acc[jj] += (kk[k][jj] == want && pos[k][jj]) ? gf[k][jj] : 0.0f;
                }
            }
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) acc[jj] *= sc[jj];
            if (oh < OH && ow < OW)
                *reinterpret_cast<u32x4*>(gy + ((((size_t)n * OH + oh) * OW + ow) * C8 + c8) * 8) = pack8(acc);
        }
    }
}

// =========================================================================================================== //
// stem_conv_bwd, shift form: input gradient of the 7x7/2 convolution (64 -> 3 channels), times 1/std of the normalisation.
//   g_x[ci][ih][iw] = inv_std[ci] * sum_{kh,kw,co} g_y1[(ih+3-kh)/2][(iw+3-kw)/2][co] * w[co][ci][kh][kw]
//   over the taps with even ih+3-kh, iw+3-kw: the input pixels split into 4 parity classes (A, BB) = (ih&1, iw&1) with
//   3 or 4 taps per axis.  Workgroup = 16 x 32 input pixels of one image = 4 classes x (8 x 16) pixels; wave w takes
//   sub-rows 2w, 2w+1 of every class.  MFMA roles: A = weights, B = g_y1 patches (columns = pixels; 8 consecutive co =
//   one aligned 16-byte LDS read).
// A tap of parity class (A, BB) reads g_y1 at row shift dr = (A + 3 - kh) / 2 and column shift dc = (BB + 3 - kw) / 2,
// both in {-1, 0, 1, 2}, and for a given (dr, dc) every class has at most one tap: the 49 (class, tap) pairs are 16
// shifts.  The B fragment (g_y1) depends on the shift alone, so the four classes share it and ONE MFMA per (shift,
// channel half, sub-row):
//   A row 4 * class + ci = w[co][ci][A + 3 - 2 dr][BB + 3 - 2 dc], zero where the class has no tap at this shift
//   (A = 0 with dr = 2, BB = 0 with dc = 2) and for ci = 3; C register r of lane l is row 4 * (l >> 4) + r, so lane group
//   l >> 4 ends up with class l >> 4, ci in registers 0..2, pixel column l & 15.
// 64 MFMAs per wave, 12 useful rows of 16.  Bits: walking dr = 2, 1, 0, -1 outside, dc = 2, 1, 0, -1 inside, then the
// channel half, every class meets its own taps with kh, then kw ascending (the order of a loop over one class's taps,
// which tests/golden/retired_variant_bits.json records); the MFMAs of a shift at which a class has no tap have a zero A
// row there and add an exact zero to a sum that started at +0 and so is never -0.  That holds for every finite g_y1: a
// non-finite g_y1 value turns 0 * inf into NaN at the pixels of the other classes under the same shift (adil_hip.h).
// LDS: the g_y1 tile at a pixel stride of 160 B (the 16 lanes that ds_read_b128 serves together — 8 pixels of one K
//   slice and the other 8 pixels of the next — then fall on 16 different 16-byte bank groups; at 144 B this kernel took
//   335 us instead of 296 at B = 512), and the three weight rows with padded kh and ci strides, so that the 12 rows x 4
//   K slices of an A fragment do the same.  52.7 KB: 3 workgroups per CU.
// Grid: one resident set of workgroups (3 per CU) that each walk a run of consecutive 16 x 32 tiles: the weights are
//   staged once per workgroup, not once per tile (18.8 KB next to a 26.8 KB tile), and the global loads of tile t + 1
//   are issued in front of the MFMAs of tile t and written to LDS behind them (one tile per workgroup: 296 us at
//   B = 512; this form: 246 - 262 us).
// =========================================================================================================== //
#define SB_TH 16
#define SB_TW 32
#define SB_GR (SB_TH / 2 + 3)          // 11 g_y1 rows
#define SB_GC (SB_TW / 2 + 3)          // 19 g_y1 columns
#define SQ_PS 80                       // g_y1 pixel stride (elements): 160 B
#define SQ_WKH (7 * 64 + 8)            // weight stride of kh (elements): 57 x 16 B
#define SQ_WCI (7 * SQ_WKH + 24)       // weight stride of ci (elements): 402 x 16 B
#define SQ_WN (2 * SQ_WCI + 6 * SQ_WKH + 7 * 64)   // weight image, followed by one zero chunk

// v_mfma_f32_16x16x32_bf16: A lane l -> row l&15, k = 8*(l>>4)+j; B lane l -> column l&15, same k; C register r of
// lane l -> row 4*(l>>4)+r, column l&15 (layout checked on hardware): 16 pixels x 32 channels of K per instruction
// (f32x4: adil_first_patch.h).

template <typename TX> __device__ __forceinline__ void st_pair(TX* p, float a, float b);
template <> __device__ __forceinline__ void st_pair<float>(float* p, float a, float b) {
    *reinterpret_cast<float2*>(p) = make_float2(a, b);
}
template <> __device__ __forceinline__ void st_pair<bf16_t>(bf16_t* p, float a, float b) {
    *reinterpret_cast<unsigned*>(p) = pack2_bf16(a, b);
}

template <typename TX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void stem_conv_bwd_shift_kernel(
    const bf16_t* __restrict__ gy, const bf16_t* __restrict__ wb, InputNorm nm, TX* __restrict__ gx, int H, int W, int OH,
    int OW, int NTX, int NTY, int ntiles) {
    __shared__ __attribute__((aligned(16))) bf16_t sg[SB_GR * SB_GC * SQ_PS];
    __shared__ __attribute__((aligned(16))) bf16_t swb[SQ_WN + 8];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int NWQ = (3 * 49 * 8 + 255) / 256, NGQ = (SB_GR * SB_GC * 8 + 255) / 256;
    // tiles in the order x, y, image; workgroup i of G takes the consecutive tiles [i ntiles / G, (i + 1) ntiles / G)
    const int t0 = (int)((long long)blockIdx.x * ntiles / gridDim.x), t1 = (int)((long long)(blockIdx.x + 1) * ntiles / gridDim.x);
    int n, ih0, iw0;                                       // the tile being computed
    u32x4 gv[NGQ];                                         // the g_y1 tile on its way from global memory to LDS
    unsigned gok = 0;
    // every global load of a tile is in flight before the first LDS store; the loads of tile t + 1 are issued in front
    // of the MFMAs of tile t and land in LDS behind them
    auto tile_load = [&](int t, int& tn, int& tih0, int& tiw0) {
        const int tx = t % NTX, r = t / NTX;
        tn = r / NTY;
        tih0 = (r - tn * NTY) * SB_TH;
        tiw0 = tx * SB_TW;
        const int ohb = tih0 / 2 - 1, owb = tiw0 / 2 - 1;
        gok = 0;
#pragma unroll
        for (int j = 0; j < NGQ; ++j) {
            const int q = tid + 256 * j < SB_GR * SB_GC * 8 ? tid + 256 * j : SB_GR * SB_GC * 8 - 1;
            const int ch = q & 7, px = q >> 3;
            const int row = px / SB_GC, col = px - row * SB_GC;
            const int oh = ohb + row, ow = owb + col;
            const bool ok = (oh >= 0) && (oh < OH) && (ow >= 0) && (ow < OW);
            gok |= ok ? 1u << j : 0u;
            gv[j] = *reinterpret_cast<const u32x4*>(gy + (((size_t)tn * OH + (ok ? oh : 0)) * OW + (ok ? ow : 0)) * 64 + ch * 8);
        }
    };
    auto tile_to_lds = [&]() {
#pragma unroll
        for (int j = 0; j < NGQ; ++j) {
            const int q = tid + 256 * j;
            const int ch = q & 7, px = q >> 3;
            u32x4 t = gv[j];
            if (!(gok >> j & 1u)) t = u32x4{0u, 0u, 0u, 0u};
            if (q < SB_GR * SB_GC * 8) *reinterpret_cast<u32x4*>(sg + px * SQ_PS + ch * 8) = t;
        }
    };
    {
        u32x4 wv[NWQ];
#pragma unroll
        for (int j = 0; j < NWQ; ++j) {
            const int q = tid + 256 * j < 3 * 49 * 8 ? tid + 256 * j : 3 * 49 * 8 - 1;
            wv[j] = *reinterpret_cast<const u32x4*>(wb + q * 8);
        }
        tile_load(t0, n, ih0, iw0);
#pragma unroll
        for (int j = 0; j < NWQ; ++j) {
            const int q = tid + 256 * j;
            const int ci = q / (49 * 8), r = q - ci * 49 * 8, tap = r >> 3, ch = r & 7, kh = tap / 7, kw = tap - kh * 7;
            if (q < 3 * 49 * 8) *reinterpret_cast<u32x4*>(swb + ci * SQ_WCI + kh * SQ_WKH + kw * 64 + ch * 8) = wv[j];
        }
        if (tid == 0) *reinterpret_cast<u32x4*>(swb + SQ_WN) = u32x4{0u, 0u, 0u, 0u};
        tile_to_lds();
    }
    lds_sync();
    const int l16 = lane & 15, ks = lane >> 4;             // B: pixel column / K slice.  A: row 4 * class + ci / K slice
    const int ci = l16 & 3, ca = l16 >> 3, cb = (l16 >> 2) & 1;
    // A fragment of shift (dr, dc), half cg: abase - 2 dr SQ_WKH - 2 dc 64 + 32 cg, or the zero chunk
    const int abase = (ci < 3 ? ci : 0) * SQ_WCI + (ca + 3) * SQ_WKH + (cb + 3) * 64 + 8 * ks;
    const bool okc = ci < 3, oka = okc && ca == 1, okb = okc && cb == 1, okab = oka && cb == 1;
    // B fragment of sub-row q: bbase + ((q + dr) SB_GC + dc) SQ_PS + 32 cg
    const int bbase = ((2 * w + 1) * SB_GC + l16 + 1) * SQ_PS + 8 * ks;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        int nn = 0, nih0 = 0, niw0 = 0;
        if (t + 1 < t1) tile_load(t + 1, nn, nih0, niw0);
        f32x4 acc[2];
        acc[0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        acc[1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        // 32 steps s = (shift, cg), the LDS reads of step s + SQ_AHEAD issued in front of the MFMAs of step s
        constexpr int SQ_AHEAD = 2;
        bf16x8 fa[SQ_AHEAD + 1], fb[SQ_AHEAD + 1][2];
#pragma unroll
        for (int s = 0; s < 32 + SQ_AHEAD; ++s) {
            if (s < 32) {
                const int dr = 2 - (s >> 3), dc = 2 - ((s >> 1) & 3), cg = s & 1, f = s % (SQ_AHEAD + 1);
                const bool ok = dr == 2 ? (dc == 2 ? okab : oka) : (dc == 2 ? okb : okc);
                fa[f] = lds8(swb + (ok ? abase - 2 * dr * SQ_WKH - 2 * dc * 64 + 32 * cg : SQ_WN));
#pragma unroll
                for (int q = 0; q < 2; ++q) fb[f][q] = lds8(sg + bbase + ((q + dr) * SB_GC + dc) * SQ_PS + 32 * cg);
            }
            if (s >= SQ_AHEAD) {
                const int f = (s - SQ_AHEAD) % (SQ_AHEAD + 1);
#pragma unroll
                for (int q = 0; q < 2; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[f], fb[f][q], acc[q], 0, 0, 0);
            }
        }
        // lane group ks holds class ks = 2 A + BB: the iw pair of one output row sits in lanes l (BB = 0) and l + 16 (BB = 1)
        const int iw = iw0 + 2 * l16;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int ih = ih0 + 2 * (2 * w + q) + (ks >> 1);
            float v[3], o[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                v[c] = acc[q][c] * nm.inv_std[c];
                o[c] = __shfl_down(v[c], 16);
            }
            if (!(ks & 1) && ih < H && iw < W) {
#pragma unroll
                for (int c = 0; c < 3; ++c) st_pair<TX>(gx + (((size_t)n * 3 + c) * H + ih) * W + iw, v[c], o[c]);
            }
        }
        if (t + 1 < t1) {                                  // uniform over the workgroup
            lds_sync();                                    // every wave is done reading tile t
            tile_to_lds();
            n = nn; ih0 = nih0; iw0 = niw0;
            lds_sync();
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------ //
extern "C" int adil_stem_conv_fwd(const void* x, int x_dtype, const void* w_fwd, float mean0, float mean1, float mean2,
                                  float inv_std0, float inv_std1, float inv_std2, const float* scale, const float* shift,
                                  void* y, int B, int H, int W, void* stream) {
    ADIL_ENTER();
    // B is blockIdx.z: beyond 65535 images the outcome would be the runtime's (a launch error code, or a launch), so refuse
    if (!x || !w_fwd || !scale || !shift || !y || B <= 0 || B > 65535 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return ADIL_EINVAL;
    if (x_dtype != ADIL_F32 && x_dtype != ADIL_BF16) return ADIL_EINVAL;
    const InputNorm nm = {{mean0, mean1, mean2}, {inv_std0, inv_std1, inv_std2}};
    const int OH = H / 2, OW = W / 2;
    const dim3 grid((OW + ST_T - 1) / ST_T, (OH + ST_T - 1) / ST_T, B);
    hipStream_t st = (hipStream_t)stream;
    if (x_dtype == ADIL_F32)
        hipLaunchKernelGGL(stem_conv_fwd_kernel<float>, grid, dim3(256), 0, st, (const float*)x, (const bf16_t*)w_fwd, nm,
                           scale, shift, (bf16_t*)y, H, W, OH, OW);
    else
        hipLaunchKernelGGL(stem_conv_fwd_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)w_fwd, nm,
                           scale, shift, (bf16_t*)y, H, W, OH, OW);
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_maxpool_fwd(const void* y, void* p, uint8_t* idx, int B, int OH, int OW, int C, void* stream) {
    ADIL_ENTER();
    if (!y || !p || !idx || B <= 0 || OH <= 0 || OW <= 0 || C <= 0 || (C & 7)) return ADIL_EINVAL;
    const int PH = (OH - 1) / 2 + 1, PW = (OW - 1) / 2 + 1;
    const size_t total = (size_t)B * PH * PW * (C / 8);
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)y, (bf16_t*)p, idx, B, OH, OW, PH, PW, C / 8);
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_stem_pool_bwd(const void* g, const uint8_t* idx, const void* p, const float* scale, void* gy, int B,
                                  int OH, int OW, int C, void* stream) {
    ADIL_ENTER();
    if (!g || !idx || !p || !scale || !gy || B <= 0 || OH <= 0 || OW <= 0 || C <= 0 || (C & 7)) return ADIL_EINVAL;
    const int PH = (OH - 1) / 2 + 1, PW = (OW - 1) / 2 + 1;
    // (n, a) is blockIdx.x and a chunk of 256 (b, c8) blockIdx.y: a grid beyond either limit is refused
    const long long rows = (long long)B * PH, cols = ((long long)PW * (C / 8) + 255) / 256;
    if (rows > 0x7fffffffLL || cols > 65535) return ADIL_EINVAL;
    hipLaunchKernelGGL(stem_pool_bwd_quad_kernel, dim3((unsigned)rows, (unsigned)cols), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)g, idx, (const bf16_t*)p, scale, (bf16_t*)gy, OH, OW, PH, PW, C / 8);
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_stem_conv_bwd(const void* gy, const void* w_bwd, float inv_std0, float inv_std1, float inv_std2, void* gx,
                                  int gx_dtype, int B, int H, int W, void* stream) {
    ADIL_ENTER();
    if (!gy || !w_bwd || !gx || B <= 0 || B > 65535 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return ADIL_EINVAL;   // as the forward
    if (gx_dtype != ADIL_F32 && gx_dtype != ADIL_BF16) return ADIL_EINVAL;
    const InputNorm nm = {{0.0f, 0.0f, 0.0f}, {inv_std0, inv_std1, inv_std2}};
    const int OH = H / 2, OW = W / 2;
    const int NTX = (W + SB_TW - 1) / SB_TW, NTY = (H + SB_TH - 1) / SB_TH;
    const long long ntiles = (long long)NTX * NTY * B;
    if (ntiles > 0x7fffffffLL) return ADIL_EINVAL;               // the kernel numbers its tiles with 32 bits
    hipStream_t st = (hipStream_t)stream;
    // one resident set of workgroups (3 per CU), each walking its share of the tiles: the weights are staged once per
    // workgroup and the g_y1 loads of a tile run under the MFMAs of the tile before it
    const long long slots = 3LL * adil_num_cu();
    const dim3 lin((unsigned)(ntiles < slots ? ntiles : slots));
    if (gx_dtype == ADIL_F32)
        hipLaunchKernelGGL(stem_conv_bwd_shift_kernel<float>, lin, dim3(256), 0, st, (const bf16_t*)gy, (const bf16_t*)w_bwd, nm,
                           (float*)gx, H, W, OH, OW, NTX, NTY, (int)ntiles);
    else
        hipLaunchKernelGGL(stem_conv_bwd_shift_kernel<bf16_t>, lin, dim3(256), 0, st, (const bf16_t*)gy, (const bf16_t*)w_bwd,
                           nm, (bf16_t*)gx, H, W, OH, OW, NTX, NTY, (int)ntiles);
    ADIL_CHECK_LAUNCH();
    return 0;
}
