// adil_bias_relu_pool2.hip — what follows a raw 3x3 convolution (adil_conv3x3.hip) in a pooled group of a frozen VGG (gfx950):
//   bias_relu_pool2 fwd / bwd  bias + ReLU + 2x2 / stride 2 max-pool in one pass, and its input gradient from a byte index
// Contracts: include/adil_hip.h.
#include "adil_mfma.h"

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
