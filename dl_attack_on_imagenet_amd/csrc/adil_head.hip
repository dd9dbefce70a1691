// adil_head.hip — global average pooling + the last linear layer of the frozen classifier with fp32 logits, forward and
// input gradient, on the channels_last bf16 activation itself: adil_pool_head_fwd / adil_pool_head_bwd
// (include/adil_hip.h).  x and gx are [B][HW][C] bf16; everything behind the pool is fp32.
//
// Two launches per call, a stream pass and a small GEMM:
//   head_pool_kernel    workgroup (256 threads) = 32 lanes x 8 rows on ONE image: a lane owns 8 channels (one 16-byte load
//                       per pixel), a row takes the pixels hw = r, r + 8, ...; four loads are in flight per thread.  The
//                       8 row sums meet in LDS in a fixed order (r = 0 .. 7), the sum is multiplied by 1 / HW once and
//                       written as fp32.  Grid = ceil(C / 256) x B: 2560 workgroups at B = 512, C = 1280, so the pass
//                       fills the chip whatever HW is; x is read once.
//   head_spread_kernel  the same decomposition the other way: a lane reads its 8 gpooled values once, multiplies them by
//                       1 / HW, rounds to bf16 and writes the same 16 bytes to every pixel of its row set; gx is written
//                       once.
//   head_gemm_kernel    out[M][N] = a[M][K] . b[K][N] (+ bias[n]) on fp32 operands with plain fp32 FMAs (1.3 GFLOP at the
//                       workload shape: the vector ALU does that in microseconds, and the products stay exact fp32
//                       products).  Serves both directions: logits = pooled . wt + bias (K = C, N = classes) and
//                       gpooled = g . w (K = classes, N = C), in both of which the second operand is read along its
//                       contiguous index.  Workgroup = a 64 x 64 tile, a thread = 4 x 4 outputs, K in steps of 16 through
//                       LDS with the next step's global loads in flight during the FMAs.  16-byte loads / stores where K
//                       resp. N is a multiple of 4, element-wise ones otherwise (any number of classes is correct, the
//                       multiples of 4 are fast).
//   head_bn_pool_kernel / head_bn_spread_kernel   the two stream passes behind an eval-BatchNorm + ReLU (DenseNet-121's norm5):
//                       adil_bn_pool_head_fwd / adil_bn_pool_head_bwd.  The same decomposition; a lane loads its 8 pscale /
//                       pshift values once, the forward sums the un-rounded max(pw_preact(x), 0), the gradient reads x once
//                       more, recomputes the branch and masks the packed bf16 words of its value.
// Nothing outside an operand's extents is loaded: every tail (images, channel chunks, pixels, K, N) is predicated.
// Offsets are 64-bit; no atomics: the summation order is fixed by the decomposition, so results are reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adil_common.h"
#include "adil_hip.h"
#include "adil_mfma.h"
#include "adil_pw_tile.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define PH_CL 32                       // 16-byte channel chunks per workgroup (256 channels)
#define PH_R 8                         // pixel rows per workgroup
#define PH_CH (PH_CL * 8)              // channels per workgroup

__global__ __launch_bounds__(256) void head_pool_kernel(const bf16_t* __restrict__ x, float* __restrict__ pooled, int HW, int C,
                                                        float inv_hw) {
    __shared__ __attribute__((aligned(16))) float part[PH_R][PH_CH];
    const int tid = threadIdx.x, cl = tid & (PH_CL - 1), r = tid >> 5;
    const int b = blockIdx.y, c = (blockIdx.x * PH_CL + cl) * 8;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
    if (c < C) {
        const bf16_t* p = x + (size_t)b * (size_t)HW * (size_t)C + (size_t)c;
        int hw = r;
        for (; hw + 3 * PH_R < HW; hw += 4 * PH_R) {
            u32x4 t[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = *reinterpret_cast<const u32x4*>(p + (size_t)(hw + j * PH_R) * (size_t)C);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float f[8];
                unpack8(t[j], f);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += f[e];
            }
        }
        for (; hw < HW; hw += PH_R) {
            float f[8];
            unpack8(*reinterpret_cast<const u32x4*>(p + (size_t)hw * (size_t)C), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += f[e];
        }
    }
    *reinterpret_cast<f32x4*>(&part[r][cl * 8]) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4*>(&part[r][cl * 8 + 4]) = f32x4{acc[4], acc[5], acc[6], acc[7]};
    lds_sync();
    const int co = blockIdx.x * PH_CH + tid;
    if (co < C) {
        float s = part[0][tid];
#pragma unroll
        for (int q = 1; q < PH_R; ++q) s += part[q][tid];
        pooled[(size_t)b * (size_t)C + (size_t)co] = s * inv_hw;
    }
}

__global__ __launch_bounds__(256) void head_spread_kernel(const float* __restrict__ gpooled, bf16_t* __restrict__ gx, int HW,
                                                          int C, float inv_hw) {
    const int tid = threadIdx.x, cl = tid & (PH_CL - 1), r = tid >> 5;
    const int b = blockIdx.y, c = (blockIdx.x * PH_CL + cl) * 8;
    if (c >= C) return;
    const float* gp = gpooled + (size_t)b * (size_t)C + (size_t)c;
    const f32x4 lo = *reinterpret_cast<const f32x4*>(gp), hi = *reinterpret_cast<const f32x4*>(gp + 4);
    const float f[8] = {lo[0] * inv_hw, lo[1] * inv_hw, lo[2] * inv_hw, lo[3] * inv_hw,
                        hi[0] * inv_hw, hi[1] * inv_hw, hi[2] * inv_hw, hi[3] * inv_hw};
    const u32x4 t = pack8(f);
    bf16_t* p = gx + (size_t)b * (size_t)HW * (size_t)C + (size_t)c;
    for (int hw = r; hw < HW; hw += PH_R) *reinterpret_cast<u32x4*>(p + (size_t)hw * (size_t)C) = t;
}

// ---- the same two passes behind an eval-BatchNorm + ReLU (DenseNet's norm5): adil_bn_pool_head_fwd / _bwd.  Kernels of
// their own, so the plain pair above keeps its code and its bits.

// a lane's 8 entries of a [C] fp32 table
__device__ __forceinline__ void head_table8(const float* __restrict__ t, int c, float (&f)[8]) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(t + c), hi = *reinterpret_cast<const f32x4*>(t + c + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[e] = lo[e];
        f[4 + e] = hi[e];
    }
}

// acc += max(pre, 0) on the 8 channels of one pixel; pre <= 0 (and -0.0, and NaN) adds +0.  Nothing is rounded to bf16
__device__ __forceinline__ void head_bn_relu_add(const u32x4& t, const float (&ps)[8], const float (&pb)[8], float (&acc)[8]) {
    float f[8];
    unpack8(t, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float pre = pw_preact(f[e], ps[e], pb[e]);
        acc[e] += pre > 0.0f ? pre : 0.0f;
    }
}

// head_pool_kernel with p = max(pw_preact(x, pscale, pshift), 0) in place of x: same decomposition, same summation order
__global__ __launch_bounds__(256) void head_bn_pool_kernel(const bf16_t* __restrict__ x, const float* __restrict__ pscale,
                                                           const float* __restrict__ pshift, float* __restrict__ pooled,
                                                           int HW, int C, float inv_hw) {
    __shared__ __attribute__((aligned(16))) float part[PH_R][PH_CH];
    const int tid = threadIdx.x, cl = tid & (PH_CL - 1), r = tid >> 5;
    const int b = blockIdx.y, c = (blockIdx.x * PH_CL + cl) * 8;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
    if (c < C) {
        float ps[8], pb[8];
        head_table8(pscale, c, ps);
        head_table8(pshift, c, pb);
        const bf16_t* p = x + (size_t)b * (size_t)HW * (size_t)C + (size_t)c;
        int hw = r;
        for (; hw + 3 * PH_R < HW; hw += 4 * PH_R) {
            u32x4 t[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = *reinterpret_cast<const u32x4*>(p + (size_t)(hw + j * PH_R) * (size_t)C);
#pragma unroll
            for (int j = 0; j < 4; ++j) head_bn_relu_add(t[j], ps, pb, acc);
        }
        for (; hw < HW; hw += PH_R) head_bn_relu_add(*reinterpret_cast<const u32x4*>(p + (size_t)hw * (size_t)C), ps, pb, acc);
    }
    *reinterpret_cast<f32x4*>(&part[r][cl * 8]) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4*>(&part[r][cl * 8 + 4]) = f32x4{acc[4], acc[5], acc[6], acc[7]};
    lds_sync();
    const int co = blockIdx.x * PH_CH + tid;
    if (co < C) {
        float s = part[0][tid];
#pragma unroll
        for (int q = 1; q < PH_R; ++q) s += part[q][tid];
        pooled[(size_t)b * (size_t)C + (size_t)co] = s * inv_hw;
    }
}

// v masked by the forward's branch of one pixel: the packed bf16 words are AND-ed, as in tr_bwd_kernel's epilogue
__device__ __forceinline__ u32x4 head_bn_mask(const u32x4& xr, const u32x4& v, const float (&ps)[8], const float (&pb)[8]) {
    float f[8];
    unpack8(xr, f);
    u32x4 o = v;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned lo = pw_preact(f[2 * k], ps[2 * k], pb[2 * k]) > 0.0f ? 0x0000ffffu : 0u;
        const unsigned hi = pw_preact(f[2 * k + 1], ps[2 * k + 1], pb[2 * k + 1]) > 0.0f ? 0xffff0000u : 0u;
        o[k] &= lo | hi;
    }
    return o;
}

// head_spread_kernel behind the BatchNorm + ReLU: v = bf16((gpooled inv_hw) pscale) once per lane, then x is read once and
// gx written once, v where that pixel's pre > 0 and +0 elsewhere
__global__ __launch_bounds__(256) void head_bn_spread_kernel(const float* __restrict__ gpooled, const bf16_t* __restrict__ x,
                                                             const float* __restrict__ pscale, const float* __restrict__ pshift,
                                                             bf16_t* __restrict__ gx, int HW, int C, float inv_hw) {
    const int tid = threadIdx.x, cl = tid & (PH_CL - 1), r = tid >> 5;
    const int b = blockIdx.y, c = (blockIdx.x * PH_CL + cl) * 8;
    if (c >= C) return;
    float ps[8], pb[8], f[8];
    head_table8(pscale, c, ps);
    head_table8(pshift, c, pb);
    head_table8(gpooled + (size_t)b * (size_t)C, c, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (f[e] * inv_hw) * ps[e];          // two products, each rounded, in this order
    const u32x4 v = pack8(f);
    const size_t base = (size_t)b * (size_t)HW * (size_t)C + (size_t)c;
    const bf16_t* p = x + base;
    bf16_t* q = gx + base;
    int hw = r;
    for (; hw + 3 * PH_R < HW; hw += 4 * PH_R) {
        u32x4 t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = *reinterpret_cast<const u32x4*>(p + (size_t)(hw + j * PH_R) * (size_t)C);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<u32x4*>(q + (size_t)(hw + j * PH_R) * (size_t)C) = head_bn_mask(t[j], v, ps, pb);
    }
    for (; hw < HW; hw += PH_R) {
        const size_t o = (size_t)hw * (size_t)C;
        *reinterpret_cast<u32x4*>(q + o) = head_bn_mask(*reinterpret_cast<const u32x4*>(p + o), v, ps, pb);
    }
}

// =========================================================================================================== //
#define HG_T 64                       // output tile edge (rows and columns)
#define HG_K 16                        // K step
#define HG_AS (HG_T + 4)               // row stride of the transposed a tile (floats): 272 B = 17 x 16 B

struct HeadTile { f32x4 a, b; };

// this thread's share of the K step at k0: a[m0 + tid / 4][k0 + 4 (tid % 4) ..+3] and b[k0 + tid / 16][n0 + 4 (tid % 16) ..+3],
// zeros outside the extents
template <bool AVEC, bool BVEC>
__device__ __forceinline__ HeadTile head_load(const float* __restrict__ a, const float* __restrict__ b, int M, int K, int N,
                                              int m0, int n0, int k0, int tid) {
    HeadTile t;
    t.a = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    t.b = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int am = m0 + (tid >> 2), ak = k0 + 4 * (tid & 3);
    if (am < M) {
        const float* ap = a + (size_t)am * (size_t)K + (size_t)ak;
        if (AVEC) {
            if (ak < K) t.a = *reinterpret_cast<const f32x4*>(ap);       // K % 4 == 0: all four inside
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ak + j < K) t.a[j] = ap[j];
        }
    }
    const int bk = k0 + (tid >> 4), bn = n0 + 4 * (tid & 15);
    if (bk < K) {
        const float* bp = b + (size_t)bk * (size_t)N + (size_t)bn;
        if (BVEC) {
            if (bn < N) t.b = *reinterpret_cast<const f32x4*>(bp);       // N % 4 == 0: all four inside
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (bn + j < N) t.b[j] = bp[j];
        }
    }
    return t;
}

template <bool AVEC, bool BVEC>
__global__ __launch_bounds__(256) void head_gemm_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        const float* __restrict__ bias, float* __restrict__ out, int M,
                                                        int K, int N) {
    __shared__ __attribute__((aligned(16))) float sa[HG_K * HG_AS];      // [k][m]
    __shared__ __attribute__((aligned(16))) float sb[HG_K * HG_T];       // [k][n]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * HG_T, n0 = blockIdx.x * HG_T;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
    HeadTile t = head_load<AVEC, BVEC>(a, b, M, K, N, m0, n0, 0, tid);
    for (int k0 = 0; k0 < K; k0 += HG_K) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sa[(4 * (tid & 3) + j) * HG_AS + (tid >> 2)] = t.a[j];
        *reinterpret_cast<f32x4*>(sb + (tid >> 4) * HG_T + 4 * (tid & 15)) = t.b;
        lds_sync();
        if (k0 + HG_K < K) t = head_load<AVEC, BVEC>(a, b, M, K, N, m0, n0, k0 + HG_K, tid);
#pragma unroll
        for (int kk = 0; kk < HG_K; ++kk) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(sa + kk * HG_AS + 4 * ty);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(sb + kk * HG_T + 4 * tx);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
        lds_sync();
    }
    const int n = n0 + 4 * tx;
    float bz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n + j < N) bz[j] = bias[n + j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + 4 * ty + i;
        if (m >= M) continue;
        float* op = out + (size_t)m * (size_t)N + (size_t)n;
        if (BVEC) {
            if (n < N) *reinterpret_cast<f32x4*>(op) = f32x4{acc[i][0] + bz[0], acc[i][1] + bz[1], acc[i][2] + bz[2], acc[i][3] + bz[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n + j < N) op[j] = acc[i][j] + bz[j];
        }
    }
}

// out[M][N] = a[M][K] . b[K][N] (+ bias)
void head_gemm(const float* a, const float* b, const float* bias, float* out, int M, int K, int N, hipStream_t st) {
    const dim3 grid((N + HG_T - 1) / HG_T, (M + HG_T - 1) / HG_T), block(256);
    const bool av = K % 4 == 0, bv = N % 4 == 0;
    if (av && bv) hipLaunchKernelGGL((head_gemm_kernel<true, true>), grid, block, 0, st, a, b, bias, out, M, K, N);
    else if (av) hipLaunchKernelGGL((head_gemm_kernel<true, false>), grid, block, 0, st, a, b, bias, out, M, K, N);
    else if (bv) hipLaunchKernelGGL((head_gemm_kernel<false, true>), grid, block, 0, st, a, b, bias, out, M, K, N);
    else hipLaunchKernelGGL((head_gemm_kernel<false, false>), grid, block, 0, st, a, b, bias, out, M, K, N);
}

inline bool head_args_ok(int B, int HW, int C, int N) {
    // gridDim.y carries the image index in the stream passes
    return B >= 1 && B <= 65535 && HW >= 1 && HW <= 65536 && C >= 8 && C <= 2048 && C % 8 == 0 && N >= 1 && N <= 65535;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------ //
extern "C" int adil_pool_head_fwd(const void* x, const float* wt, const float* bias, float* pooled, float* logits, int B,
                                  int HW, int C, int N, void* stream) {
    if (!x || !wt || !bias || !pooled || !logits || !head_args_ok(B, HW, C, N)) return ADIL_EINVAL;
    if (!aligned(x, 16) || !aligned(wt, 16) || !aligned(bias, 4) || !aligned(pooled, 16) || !aligned(logits, 16))
        return ADIL_EINVAL;
    ADIL_ENTER();
    hipStream_t st = (hipStream_t)stream;
    const float inv_hw = 1.0f / (float)HW;
    const dim3 grid((C + PH_CH - 1) / PH_CH, B), block(256);
    hipLaunchKernelGGL(head_pool_kernel, grid, block, 0, st, (const bf16_t*)x, pooled, HW, C, inv_hw);
    ADIL_CHECK_LAUNCH();
    head_gemm(pooled, wt, bias, logits, B, C, N, st);
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_pool_head_bwd(const float* g, const float* w, float* gpooled, void* gx, int B, int HW, int C, int N,
                                  void* stream) {
    if (!g || !w || !gpooled || !gx || !head_args_ok(B, HW, C, N)) return ADIL_EINVAL;
    if (!aligned(g, 16) || !aligned(w, 16) || !aligned(gpooled, 16) || !aligned(gx, 16)) return ADIL_EINVAL;
    ADIL_ENTER();
    hipStream_t st = (hipStream_t)stream;
    const float inv_hw = 1.0f / (float)HW;
    head_gemm(g, w, nullptr, gpooled, B, N, C, st);
    ADIL_CHECK_LAUNCH();
    const dim3 grid((C + PH_CH - 1) / PH_CH, B), block(256);
    hipLaunchKernelGGL(head_spread_kernel, grid, block, 0, st, (const float*)gpooled, (bf16_t*)gx, HW, C, inv_hw);
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_bn_pool_head_fwd(const void* x, const float* pscale, const float* pshift, const float* wt, const float* bias,
                                     float* pooled, float* logits, int B, int HW, int C, int N, void* stream) {
    if (!x || !pscale || !pshift || !wt || !bias || !pooled || !logits || !head_args_ok(B, HW, C, N)) return ADIL_EINVAL;
    if (!aligned(x, 16) || !aligned(pscale, 16) || !aligned(pshift, 16) || !aligned(wt, 16) || !aligned(bias, 4) ||
        !aligned(pooled, 16) || !aligned(logits, 16))
        return ADIL_EINVAL;
    ADIL_ENTER();
    hipStream_t st = (hipStream_t)stream;
    const float inv_hw = 1.0f / (float)HW;
    const dim3 grid((C + PH_CH - 1) / PH_CH, B), block(256);
    hipLaunchKernelGGL(head_bn_pool_kernel, grid, block, 0, st, (const bf16_t*)x, pscale, pshift, pooled, HW, C, inv_hw);
    ADIL_CHECK_LAUNCH();
    head_gemm(pooled, wt, bias, logits, B, C, N, st);
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_bn_pool_head_bwd(const float* g, const float* w, const void* x, const float* pscale, const float* pshift,
                                     float* gpooled, void* gx, int B, int HW, int C, int N, void* stream) {
    if (!g || !w || !x || !pscale || !pshift || !gpooled || !gx || !head_args_ok(B, HW, C, N)) return ADIL_EINVAL;
    if (!aligned(g, 16) || !aligned(w, 16) || !aligned(x, 16) || !aligned(pscale, 16) || !aligned(pshift, 16) ||
        !aligned(gpooled, 16) || !aligned(gx, 16))
        return ADIL_EINVAL;
    ADIL_ENTER();
    hipStream_t st = (hipStream_t)stream;
    const float inv_hw = 1.0f / (float)HW;
    head_gemm(g, w, nullptr, gpooled, B, N, C, st);
    ADIL_CHECK_LAUNCH();
    const dim3 grid((C + PH_CH - 1) / PH_CH, B), block(256);
    hipLaunchKernelGGL(head_bn_spread_kernel, grid, block, 0, st, (const float*)gpooled, (const bf16_t*)x, pscale, pshift,
                       (bf16_t*)gx, HW, C, inv_hw);
    ADIL_CHECK_LAUNCH();
    return 0;
}
