// adil_convs.hip — the frozen ResNet's convolutions behind the stem, on channels_last bf16 storage (gfx950):
//   pw_conv_fwd / pw_conv_bwd   1x1 convolutions (stride 1, and the stride-2 downsample ones through an in-kernel
//                               gather) as GEMMs with the BatchNorm / residual / ReLU epilogue (and
//                               the previous layer's BatchNorm + ReLU as a prologue) applied on chip, forward and input
//                               gradient (both at 64 / 128 output channels per workgroup, or at 256 / 512 in an
//                               8-wave form that prepares its operand once: a measured table per direction picks the
//                               tile, and every tile gives the same bits)
//   pw_join                     conv3 of a bottleneck and conv1 of the next one as one kernel, forward and input
//                               gradient (the C-channel tensor between them stays on chip)
//   conv3x3_s2                  3x3 / stride-2 convolutions as tap-GEMMs, forward and input gradient (the stride-1 ones:
//                               adil_conv3x3.hip)
// Not part of the ADiL maths: the parity target is plain PyTorch (tests/test_gpu_stem.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adil_common.h"
#include "adil_hip.h"
#include "adil_mfma.h"

// =========================================================================================================== //
// Pointwise (1x1, stride 1) convolution of the frozen ResNet with its eval-BatchNorm / residual / ReLU epilogue
// in ONE kernel.  On channels_last storage the convolution is the row-major GEMM
//     Y[M][N] = act( (X[M][K] . W[N][K]^T) * scale[n] + shift[n] (+ R[M][N]) ),   M = B*H*W, K = Cin, N = Cout
// and at ResNet-50 / B = 512 it is HBM-bound (K <= 2048, activations of 0.1 - 0.8 GB): what matters is that every
// activation crosses HBM once.  A library GEMM + a separate epilogue kernel writes and re-reads the pre-activation
// tensor (the epilogue passes were 10.5 ms of a 51 ms step); here the epilogue runs on the accumulators.
//   Workgroup = 128 pixels x BN channels (BN = 128 or 64), K in chunks of 64 through LDS (the next chunk waits in
//   registers: one 37 KB buffer, 3-4 workgroups per CU); or BN = 256 / 512 with 8 waves and double-buffered tiles, one
//   workgroup per CU (see pw_conv_fwd_kernel).
//   MFMA roles as in the stem: A = W (rows = channels -> accumulator registers), B = X (columns = pixels -> lanes),
//   so a lane owns 4 consecutive channels of one pixel per register quad (8-byte residual loads); the finished tile
//   goes through a per-wave LDS transpose to 16-byte NHWC stores.
// =========================================================================================================== //
namespace {

#define PW_BM 128
#define PW_BK 64
#define PW_LS (PW_BK + 8)              // LDS row stride (elements): 144 B = 9 x 16 B
#define PW_PK 512                      // most input channels a fused prologue / backward epilogue supports

// The arithmetic of the prologue and of the epilogue, in ONE place for every tile: the multiply-adds are written as fused
// operations (what -ffp-contract=fast made of `a * b + c` in the 128 / 64 tiles), so no instantiation is left to contract
// on its own (FINDINGS.md 31) and every tile rounds at the same points.
//   prologue: x' = relu(bf16(fma(x, pscale, pshift)))
__device__ __forceinline__ unsigned pw_fwd_pro2(unsigned x2, f32x2 ps, f32x2 pb) {
    return relu_bf2(f32x2_to_bf2(__builtin_elementwise_fma(bf2_to_f32x2(x2), ps, pb)));
}
//   epilogue of one register quad (4 consecutive channels of one pixel): fma(acc, scale, shift), + res, round, ReLU
template <bool RES>
__device__ __forceinline__ u32x2 pw_fwd_epi4(const f32x16& acc, int q, const f32x2* sc, const f32x2* sh, u32x2 r, int relu) {
    f32x2 v0 = __builtin_elementwise_fma(f32x2{acc[4 * q], acc[4 * q + 1]}, sc[0], sh[0]);
    f32x2 v1 = __builtin_elementwise_fma(f32x2{acc[4 * q + 2], acc[4 * q + 3]}, sc[1], sh[1]);
    if (RES) {
        v0 += bf2_to_f32x2(r[0]);
        v1 += bf2_to_f32x2(r[1]);
    }
    u32x2 t;
    t[0] = f32x2_to_bf2(v0);
    t[1] = f32x2_to_bf2(v1);
    if (relu) { t[0] = relu_bf2(t[0]); t[1] = relu_bf2(t[1]); }
    return t;
}

// NW = 4 waves: each owns 32 pixels x BN channels (BN = 64, 128), one LDS buffer, 3 - 4 workgroups per CU.
//   The conv3 form <128, PRO, RES> is a stream of short workgroups (K <= 512: 1 - 8 chunks, then a 32 KB residual and a
//   32 KB store each) whose phases overlap only across workgroups, so what it needs is residents: with the residual
//   held in registers under the whole K loop it took 186 registers = 2 workgroups per CU and ran at 1.9 - 4.3 TB/s;
//   requested in front of the last chunk's MFMAs instead it takes 154 = 3 per CU: 433 -> 376, 227 -> 207, 156 -> 132 and
//   119 -> 102 us on the four conv3 shapes of ResNet-50 at B = 512 (FINDINGS.md 43).
// NW = 8 (the wide tiles, BN = 256 and 512): 4 pixel groups x 2 channel halves, ONE workgroup per CU, so the X chunk is
// loaded, run through the prologue and written to LDS once for 256 or 512 output channels instead of once per 128.
//   BN = 256 keeps two buffers of both tiles (2 x 54 KB): one barrier per chunk, chunk i + 1 is written while the waves
//   that are behind still multiply chunk i, and the loads of chunk i + 2 fly under the MFMAs of chunk i + 1.
//   BN = 512 (72 KB of W tile) keeps two buffers of the X tile only (2 x 18 KB): the prologue and the X stores of chunk
//   i + 1 overlap the other waves' MFMAs, the W stores sit between the two barriers.  Its 128 accumulators leave no room
//   for a residual under the K loop (64 registers): the residual is requested in front of the last chunk's MFMAs.
// Each output element sees the same MFMA sequence and the same epilogue at every tile: the results are bitwise the same.
template <int BN, bool PRO, bool RES, int NW>
__global__ __launch_bounds__(NW * 64)
__attribute__((amdgpu_waves_per_eu(NW == 8 ? 2 : (PRO && BN == 128 && !RES ? 2 : (RES ? 3 : 4))))) void pw_conv_fwd_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ wgt, const float* __restrict__ scale,
    const float* __restrict__ shift, const bf16_t* __restrict__ res, bf16_t* __restrict__ y, int M, int K, int N,
    int relu, int MT, int NT, const float* __restrict__ pscale, const float* __restrict__ pshift, int sub_w, int sub_hw) {
    constexpr int NTH = NW * 64;                         // threads
    constexpr int BW = BN / (NW / 4);                    // channels per wave
    constexpr int CT = BW / 32;                          // channel tiles per wave
    constexpr int XCH = PW_BM * PW_BK / 8 / NTH;         // 16-byte chunks of the X tile per thread (4; 2 with 8 waves)
    constexpr int WCH = BN * PW_BK / 8 / NTH;            // ... of the W tile (2, 4; 4, 8 with 8 waves)
    constexpr int OS = BN + 8;                           // transposed-output pixel stride (elements)
    constexpr bool DB = NW == 8 && BN == 256;            // two buffers of both tiles
    constexpr bool DX = NW == 8 && BN == 512;            // two buffers of the X tile, one of the W tile
    constexpr int XTE = PW_BM * PW_LS;                   // elements of an X tile
    constexpr int XBS = DB ? (PW_BM + BN) * PW_LS : XTE; // from one X buffer to the other
    constexpr int WBS = DB ? (PW_BM + BN) * PW_LS : 0;   // from one W buffer to the other
    // the residual is requested under the last chunk only: where 64 registers of it do not fit (BN = 512), and in the
    // conv3 form of the 128 tile, where 32 registers less are a third resident workgroup
    constexpr bool LATE = RES && (CT > 4 || (PRO && BN == 128));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sx = reinterpret_cast<bf16_t*>(smem_raw);    // [128][PW_LS]   (NW = 4: single buffer, the next chunk waits in
    bf16_t* sw = sx + (DX ? 2 : 1) * XTE;                // [BN][PW_LS]     registers; 37 KB -> 3-4 workgroups per CU)
    // w = pixel group, wc = channel half.  Spelled per NW: with 4 waves `(tid >> 6) & 3` is not folded to `tid >> 6`, and
    // the mask alone cost the narrow tiles two more spilled registers and 7 - 15 % of their time on the K >= 256 shapes
    const int tid = threadIdx.x, lane = tid & 63, w = NW == 8 ? (tid >> 6) & 3 : tid >> 6, wc = NW == 8 ? tid >> 8 : 0;
    const int c = lane & 31, h = lane >> 5;
    // workgroups are dealt round-robin to the 8 XCDs: consecutive workgroups of ONE XCD share the pixel tile, so the
    // NT reads of an X tile meet in that XCD's L2
    int mt, nt;
    if ((MT & 7) == 0) {
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        nt = j % NT;
        mt = (j / NT) * 8 + xcd;
    } else {
        nt = blockIdx.x % NT;
        mt = blockIdx.x / NT;
    }
    const int m0 = mt * PW_BM, n0 = nt * BN;
    const int nk = K / PW_BK;
    const int m = m0 + w * 32 + c;                       // this lane's pixel in the epilogue
    const bool mok = m < M;
    __shared__ __attribute__((aligned(16))) float ssc[2 * BN];   // this tile's scale | shift (visible after the first barrier)
    if (tid < BN) { ssc[tid] = scale[n0 + tid]; ssc[BN + tid] = shift[n0 + tid]; }
    // optional prologue: the X operand is the RAW output of the previous (library) convolution and its eval-BatchNorm
    // + ReLU is applied on the way from registers to LDS:  x' = relu(x * pscale[k] + pshift[k])   (K <= PW_PK)
    __shared__ __attribute__((aligned(16))) float spro[PRO ? 2 * PW_PK : 4];
    constexpr bool pro = PRO;
    if (pro) {
        const int i2 = 2 * tid < K ? 2 * tid : 0;                            // K <= 512: one float2 of each per thread
        const float2 a = *reinterpret_cast<const float2*>(pscale + i2), b = *reinterpret_cast<const float2*>(pshift + i2);
        if (2 * tid < K) {
            *reinterpret_cast<float2*>(spro + 2 * tid) = a;
            *reinterpret_cast<float2*>(spro + PW_PK + 2 * tid) = b;
        }
        __syncthreads();
    }

    // rows of X this thread stages (fixed over the K loop).  sub_w > 0: the convolution has stride 2 — output pixel
    // m = (n, oh, ow) of an (OH = sub_hw / sub_w) x (OW = sub_w) grid reads input pixel (n, 2 oh, 2 ow) of the
    // 2 OH x 2 OW tensor x points to (the stride-2 downsample convolutions gather, nothing is copied)
    size_t xrow[XCH];
#pragma unroll
    for (int i = 0; i < XCH; ++i) {
        const int id = tid + NTH * i, row = id >> 3;
        const int mm = (m0 + row < M) ? m0 + row : M - 1;
        if (sub_w > 0) {
            const int n = mm / sub_hw, r = mm - n * sub_hw, oh = r / sub_w, ow = r - oh * sub_w;
            xrow[i] = (size_t)4 * n * sub_hw + (size_t)4 * oh * sub_w + 2 * ow;
        } else {
            xrow[i] = (size_t)mm;
        }
    }
    u32x4 xr[XCH], wr[WCH];
    auto load_tiles = [&](int kc) {
#pragma unroll
        for (int i = 0; i < XCH; ++i) {
            const int id = tid + NTH * i, ch = id & 7;
            xr[i] = *reinterpret_cast<const u32x4*>(x + xrow[i] * K + kc * PW_BK + ch * 8);
        }
#pragma unroll
        for (int i = 0; i < WCH; ++i) {
            const int id = tid + NTH * i, row = id >> 3, ch = id & 7;
            wr[i] = *reinterpret_cast<const u32x4*>(wgt + (size_t)(n0 + row) * K + kc * PW_BK + ch * 8);
        }
    };
    auto store_x = [&](int kc, int buf) {
#pragma unroll
        for (int i = 0; i < XCH; ++i) {
            const int id = tid + NTH * i, row = id >> 3, ch = id & 7;
            u32x4 t = xr[i];
            if (pro) {
                const f32x2* ps = reinterpret_cast<const f32x2*>(spro + kc * PW_BK + ch * 8);
                const f32x2* pb = reinterpret_cast<const f32x2*>(spro + PW_PK + kc * PW_BK + ch * 8);
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = pw_fwd_pro2(t[j], ps[j], pb[j]);
            }
            *reinterpret_cast<u32x4*>(sx + buf * XBS + row * PW_LS + ch * 8) = t;
        }
    };
    auto store_w = [&](int buf) {
#pragma unroll
        for (int i = 0; i < WCH; ++i) {
            const int id = tid + NTH * i, row = id >> 3, ch = id & 7;
            *reinterpret_cast<u32x4*>(sw + buf * WBS + row * PW_LS + ch * 8) = wr[i];
        }
    };

    load_tiles(0);
    // the residual does not depend on the GEMM: its loads fly under the whole K loop (LATE: under the last chunk)
    u32x2 rr[RES ? CT : 1][4];
    auto load_res = [&]() {
        const bf16_t* rp = res + (size_t)(mok ? m : M - 1) * N + n0 + wc * BW + 4 * h;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int q = 0; q < 4; ++q) rr[ct][q] = *reinterpret_cast<const u32x2*>(rp + 32 * ct + 8 * q);
    };
    if (RES && !LATE) load_res();
    f32x16 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.0f;
    if (DB) {                                            // chunk 0 into buffer 0; from then on chunk it + 1 is written
        store_x(0, 0);                                   // into the other buffer after the MFMAs of chunk it
        store_w(0);
        if (1 < nk) load_tiles(1);
        lds_barrier();
    }
    if (DX) store_x(0, 0);
    for (int it = 0; it < nk; ++it) {
        if (!DB) {
            if (!DX) store_x(it, 0);
            store_w(0);
            if (it + 1 < nk) load_tiles(it + 1);
            lds_barrier();
        }
        if (LATE && it == nk - 1) load_res();
        const int cur = (DB || DX) ? (it & 1) : 0;
        const bf16_t* bx = sx + cur * XBS + (w * 32 + c) * PW_LS + 8 * h;
        const bf16_t* bw = sw + cur * WBS + (wc * BW + c) * PW_LS + 8 * h;
#pragma unroll
        for (int ks = 0; ks < PW_BK / 16; ++ks) {
            const bf16x8 b = lds8(bx + 16 * ks);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) mma16(acc[ct], lds8(bw + ct * 32 * PW_LS + 16 * ks), b);
        }
        if (DB && it + 1 < nk) {                         // nobody reads buffer cur ^ 1 in this iteration
            store_x(it + 1, cur ^ 1);
            store_w(cur ^ 1);
            if (it + 2 < nk) load_tiles(it + 2);
        }
        if (DX && it + 1 < nk) store_x(it + 1, cur ^ 1); // the X half of chunk it + 1; its W half waits for the barrier
        lds_barrier();
    }
    // epilogue on the accumulators: lane = pixel m, register quad q of tile ct = channels n0 + wc BW + 32ct + 8q + 4h .. +3
    bf16_t* so = reinterpret_cast<bf16_t*>(smem_raw) + w * 32 * OS + wc * BW;   // the tile buffers are idle now
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int co = 32 * ct + 8 * q + 4 * h;
            const f32x2* sc = reinterpret_cast<const f32x2*>(ssc + wc * BW + co);
            const f32x2* sh = reinterpret_cast<const f32x2*>(ssc + BN + wc * BW + co);
            *reinterpret_cast<u32x2*>(so + c * OS + co) = pw_fwd_epi4<RES>(acc[ct], q, sc, sh, rr[RES ? ct : 0][q], relu);
        }
    }
    constexpr int CPP = BW / 8;                           // 16-byte chunks per pixel of this wave's corner
#pragma unroll
    for (int i = 0; i < 32 * CPP / 64; ++i) {
        const int id = lane + 64 * i, px = id / CPP, ch = id - px * CPP;
        const u32x4 t = *reinterpret_cast<const u32x4*>(so + px * OS + ch * 8);
        const int mm = m0 + w * 32 + px;
        if (mm < M) *reinterpret_cast<u32x4*>(y + (size_t)mm * N + n0 + wc * BW + ch * 8) = t;
    }
}

// Input gradient of the same layer, again ONE kernel:  with v = g (+ g2), mask = [y > 0] (all ones without ReLU),
//     gres[M][N] = v * mask                      (gradient of the residual input; optional)
//     gx[M][K]   = (v * mask * scale[n]) . W     (W given transposed: wt[K][N], so the reduction index n is contiguous)
// The epilogue backward is applied to the X-operand chunk on its way from registers to LDS (it would otherwise be a
// separate kernel writing and re-reading an M x N tensor), and g2 lets the caller hand over the two gradients that
// meet at a residual join without adding them first (autograd's add kernels were 3 ms of a 46 ms step).
//   NW = 4 waves: each owns 32 pixels x BO channels (BO = 64, 128), one LDS buffer, two workgroups per CU.
//   NW = 8 (the wide tiles, BO = 256 and 512, G3 = false only): 4 pixel groups x 2 channel halves, so the operand chunk —
//   three M x N loads, the add, mask, scale and rounding of store_tiles — is prepared once for 256 or 512 output
//   channels instead of once per 128 (at K = 512, N = 2048 a narrow workgroup pulls 1.5 MB of operand through L2 for 67
//   MFLOP).  ONE workgroup of 8 waves lives on a CU (166 / 252 registers; BO = 256 with 4 waves and 128 accumulators, or
//   with 8 waves under a 128-register budget, spills).  BO = 256 double-buffers the tiles in the LDS it has to itself
//   (2 x 54 KB): one barrier per chunk, and the waves that are ahead prepare chunk i+1 while the others still multiply
//   chunk i.  BO = 512 (90 KB of tiles, 130 KB for the output transpose) keeps the single buffer.
//   Each output element sees the same MFMA sequence at every tile: the results are bitwise the same.
template <int BO, bool G3, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu((NW == 8 || BO == 128 || G3) ? 2 : 3))) void pw_conv_bwd_kernel(
    const bf16_t* __restrict__ g, const bf16_t* __restrict__ g2, const bf16_t* __restrict__ y,
    const float* __restrict__ scale, const bf16_t* __restrict__ wt, bf16_t* __restrict__ gx, bf16_t* __restrict__ gres,
    int M, int K, int N, int relu, int MT, int OT, const bf16_t* __restrict__ xin, const float* __restrict__ pscale,
    const float* __restrict__ pshift, const bf16_t* __restrict__ g3, int sub_w, int sub_hw) {
    constexpr int NT = NW * 64;                          // threads
    constexpr int BW = BO / (NW / 4);                    // output channels per wave
    constexpr int CT = BW / 32;
    constexpr int XCH = PW_BM * PW_BK / 8 / NT;          // 4 (2 with 8 waves)
    constexpr int WCH = BO * PW_BK / 8 / NT;
    constexpr int OS = BO + 8;
    constexpr bool DB = NW == 8 && BO == 256;            // two tile buffers (BO = 512: 2 x 90 KB do not fit)
    constexpr int BUFE = (PW_BM + BO) * PW_LS;           // elements of one buffer
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sx = reinterpret_cast<bf16_t*>(smem_raw);    // [128][PW_LS]  gz chunk
    bf16_t* sw = sx + PW_BM * PW_LS;                     // [BO][PW_LS]   wt chunk
    const int tid = threadIdx.x, lane = tid & 63, w = (tid >> 6) & 3, wc = tid >> 8, c = lane & 31, h = lane >> 5;
    int mt, ot;
    if ((MT & 7) == 0) {
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        ot = j % OT;
        mt = (j / OT) * 8 + xcd;
    } else {
        ot = blockIdx.x % OT;
        mt = blockIdx.x / OT;
    }
    const int m0 = mt * PW_BM, k0 = ot * BO;
    const int nn = N / PW_BK;
    const bool write_res = (gres != nullptr) && (ot == 0);
    __shared__ __attribute__((aligned(16))) float ssc[2048];     // BatchNorm scale of every reduction channel
    {   // N <= 2048 floats = at most two float4 per thread, both in flight together (a rolled scalar loop pays up to
        // eight memory round trips before the first tile load is even issued)
        float4 sv[512 / NT];
#pragma unroll
        for (int j = 0; j < 512 / NT; ++j) {
            const int i4 = tid + NT * j;
            sv[j] = *reinterpret_cast<const float4*>(scale + (4 * i4 < N ? 4 * i4 : 0));
        }
#pragma unroll
        for (int j = 0; j < 512 / NT; ++j) {
            const int i4 = tid + NT * j;
            if (4 * i4 < N) *reinterpret_cast<float4*>(ssc + 4 * i4) = sv[j];
        }
    }
    __syncthreads();

    // G3: a third incoming gradient that lives on the stride-2 grid (it comes back from a stride-2 downsample
    // convolution reading this layer's output): pixel (n, h, w) of the 2 OH x 2 OW grid receives g3[(n, h/2, w/2)] when
    // h and w are even, nothing otherwise — the zero-upsampled tensor is never materialised.
    size_t g3row[G3 ? XCH : 1];
    float g3on[G3 ? XCH : 1];
    if (G3) {
#pragma unroll
        for (int i = 0; i < XCH; ++i) {
            const int id = tid + NT * i, row = id >> 3;
            const int mm = (m0 + row < M) ? m0 + row : M - 1;
            const int hw4 = 4 * sub_hw, w2 = 2 * sub_w;
            const int n = mm / hw4, r = mm - n * hw4, hh = r / w2, ww = r - hh * w2;
            g3on[i] = ((hh | ww) & 1) ? 0.0f : 1.0f;
            g3row[i] = (size_t)n * sub_hw + (size_t)(hh >> 1) * sub_w + (ww >> 1);
        }
    }
    u32x4 gr[XCH], hr[XCH], yr[XCH], tr[G3 ? XCH : 1], wr[WCH];
    auto load_tiles = [&](int nc) {
#pragma unroll
        for (int i = 0; i < XCH; ++i) {
            const int id = tid + NT * i, row = id >> 3, ch = id & 7;
            const int mm = m0 + row;
            const size_t at = (size_t)(mm < M ? mm : M - 1) * N + nc * PW_BK + ch * 8;
            gr[i] = *reinterpret_cast<const u32x4*>(g + at);
            if (g2 != nullptr) hr[i] = *reinterpret_cast<const u32x4*>(g2 + at);
            if (relu) yr[i] = *reinterpret_cast<const u32x4*>(y + at);
            if (G3) tr[i] = *reinterpret_cast<const u32x4*>(g3 + g3row[i] * N + nc * PW_BK + ch * 8);   // always a valid address
        }
#pragma unroll
        for (int i = 0; i < WCH; ++i) {
            const int id = tid + NT * i, row = id >> 3, ch = id & 7;
            wr[i] = *reinterpret_cast<const u32x4*>(wt + (size_t)(k0 + row) * N + nc * PW_BK + ch * 8);
        }
    };
    auto store_tiles = [&](int nc, int buf) {
#pragma unroll
        for (int i = 0; i < XCH; ++i) {
            const int id = tid + NT * i, row = id >> 3, ch = id & 7;
            const f32x2* s2 = reinterpret_cast<const f32x2*>(ssc + nc * PW_BK + ch * 8);
            u32x4 rs, gz;                                             // gres chunk, gz chunk (packed bf16)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x2 v = bf2_to_f32x2(gr[i][j]);
                if (g2 != nullptr) v += bf2_to_f32x2(hr[i][j]);
                if (G3) v += bf2_to_f32x2(tr[i][j]) * g3on[i];
                const unsigned m = relu ? pos_mask_bf2(yr[i][j]) : 0xffffffffu;
                rs[j] = f32x2_to_bf2(v) & m;
                gz[j] = f32x2_to_bf2(v * s2[j]) & m;
            }
            const int mm = m0 + row;
            if (write_res && mm < M) *reinterpret_cast<u32x4*>(gres + (size_t)mm * N + nc * PW_BK + ch * 8) = rs;
            *reinterpret_cast<u32x4*>(sx + buf * BUFE + row * PW_LS + ch * 8) = gz;
        }
#pragma unroll
        for (int i = 0; i < WCH; ++i) {
            const int id = tid + NT * i, row = id >> 3, ch = id & 7;
            *reinterpret_cast<u32x4*>(sw + buf * BUFE + row * PW_LS + ch * 8) = wr[i];
        }
    };

    load_tiles(0);
    f32x16 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.0f;
    if (DB) {                                            // chunk 0 into buffer 0; from then on chunk it + 1 is written
        store_tiles(0, 0);                               // into the other buffer after the MFMAs of chunk it
        if (1 < nn) load_tiles(1);
        lds_barrier();
    }
    for (int it = 0; it < nn; ++it) {
        if (!DB) {
            store_tiles(it, 0);
            if (it + 1 < nn) load_tiles(it + 1);
            lds_barrier();
        }
        const int cur = DB ? (it & 1) : 0;
        const bf16_t* bx = sx + cur * BUFE + (w * 32 + c) * PW_LS + 8 * h;
        const bf16_t* bw = sw + cur * BUFE + (wc * BW + c) * PW_LS + 8 * h;
#pragma unroll
        for (int ks = 0; ks < PW_BK / 16; ++ks) {
            const bf16x8 b = lds8(bx + 16 * ks);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) mma16(acc[ct], lds8(bw + ct * 32 * PW_LS + 16 * ks), b);
        }
        if (DB && it + 1 < nn) {                         // nobody reads buffer cur ^ 1 in this iteration
            store_tiles(it + 1, cur ^ 1);
            if (it + 2 < nn) load_tiles(it + 2);
        }
        lds_barrier();
    }
    bf16_t* so = reinterpret_cast<bf16_t*>(smem_raw) + w * 32 * OS + wc * BW;   // this wave's 32 px x BW corner
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u32x2 t;
            t[0] = pack2_bf16(acc[ct][4 * q], acc[ct][4 * q + 1]);
            t[1] = pack2_bf16(acc[ct][4 * q + 2], acc[ct][4 * q + 3]);
            *reinterpret_cast<u32x2*>(so + c * OS + 32 * ct + 8 * q + 4 * h) = t;
        }
    }
    // optional epilogue: the forward fed this layer relu(xin * pscale + pshift) computed on the fly (xin = raw output
    // of the previous convolution), so the gradient handed back is wrt xin:  gx * [xin*pscale+pshift > 0] * pscale
    constexpr int CPP = BW / 8;
    const int kw0 = k0 + wc * BW;                        // first output channel of this wave
#pragma unroll
    for (int i = 0; i < 32 * CPP / 64; ++i) {
        const int id = lane + 64 * i, px = id / CPP, ch = id - px * CPP;
        u32x4 t = *reinterpret_cast<const u32x4*>(so + px * OS + ch * 8);
        const int mm = m0 + w * 32 + px;
        if (mm < M) {
            if (xin != nullptr) {
                float v[8], xv[8];
                unpack8(t, v);
                unpack8(*reinterpret_cast<const u32x4*>(xin + (size_t)mm * K + kw0 + ch * 8), xv);
                const float4 a0 = *reinterpret_cast<const float4*>(pscale + kw0 + ch * 8);
                const float4 a1 = *reinterpret_cast<const float4*>(pscale + kw0 + ch * 8 + 4);
                const float4 b0 = *reinterpret_cast<const float4*>(pshift + kw0 + ch * 8);
                const float4 b1 = *reinterpret_cast<const float4*>(pshift + kw0 + ch * 8 + 4);
                const float ps[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                const float pb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (xv[j] * ps[j] + pb[j] > 0.0f) ? v[j] * ps[j] : 0.0f;
                t = pack8(v);
            }
            *reinterpret_cast<u32x4*>(gx + (size_t)mm * K + kw0 + ch * 8) = t;
        }
    }
}

template <int BO, bool G3, int NW = 4>
int launch_pw_bwd(const void* g, const void* g2, const void* y, const float* scale, const void* wt, void* gx, void* gres,
                  int M, int K, int N, int relu, const void* xin, const float* pscale, const float* pshift, const void* g3,
                  int sub_w, int sub_hw, hipStream_t st) {
    const int MT = (M + PW_BM - 1) / PW_BM, OT = K / BO;
    const size_t tiles = (size_t)(NW == 8 && BO == 256 ? 2 : 1) * (PW_BM + BO) * PW_LS * sizeof(bf16_t);
    const size_t outb = (size_t)4 * 32 * (BO + 8) * sizeof(bf16_t);
    const size_t lds = tiles > outb ? tiles : outb;
    if (lds > 48 * 1024) {                               // BO = 256: 108 KB, BO = 512: 130 KB, one workgroup per CU
        const hipError_t e = hipFuncSetAttribute((const void*)pw_conv_bwd_kernel<BO, G3, NW>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((pw_conv_bwd_kernel<BO, G3, NW>), dim3((unsigned)(MT * OT)), dim3(NW * 64), lds, st, (const bf16_t*)g,
                       (const bf16_t*)g2, (const bf16_t*)y, scale, (const bf16_t*)wt, (bf16_t*)gx, (bf16_t*)gres, M, K, N,
                       relu, MT, OT, (const bf16_t*)xin, pscale, pshift, (const bf16_t*)g3, sub_w, sub_hw);
    ADIL_CHECK_LAUNCH();
    return 0;
}

template <int BN, bool PRO, bool RES>
int launch_pw_fwd_r(const void* x, const void* w, const float* scale, const float* shift, const void* res, void* y, int M,
                  int K, int N, int relu, const float* pscale, const float* pshift, int sub_w, int sub_hw, hipStream_t st) {
    constexpr int NW = BN >= 256 ? 8 : 4;
    const int MT = (M + PW_BM - 1) / PW_BM, NT = N / BN;
    // BN = 256: two buffers of both tiles; BN = 512: two X tiles and one W tile (108 KB either way)
    const size_t tiles = (size_t)(BN == 256 ? 2 * (PW_BM + BN) : (BN == 512 ? 2 * PW_BM + BN : PW_BM + BN)) * PW_LS * sizeof(bf16_t);
    const size_t outb = (size_t)4 * 32 * (BN + 8) * sizeof(bf16_t);
    const size_t lds = tiles > outb ? tiles : outb;      // BN = 512: 130 KB for the output transpose
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)pw_conv_fwd_kernel<BN, PRO, RES, NW>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((pw_conv_fwd_kernel<BN, PRO, RES, NW>), dim3((unsigned)(MT * NT)), dim3(NW * 64), lds, st, (const bf16_t*)x,
                       (const bf16_t*)w, scale, shift, (const bf16_t*)res, (bf16_t*)y, M, K, N, relu, MT, NT, pscale, pshift, sub_w, sub_hw);
    ADIL_CHECK_LAUNCH();
    return 0;
}

template <int BN>
int launch_pw_fwd(const void* x, const void* w, const float* scale, const float* shift, const void* res, void* y, int M,
                  int K, int N, int relu, const float* pscale, const float* pshift, int sub_w, int sub_hw, hipStream_t st) {
    // without a residual the 32 registers of its prefetch are free: 4 workgroups per CU instead of 3 (narrow tiles)
    if (pscale != nullptr) {
        if (res != nullptr)
            return launch_pw_fwd_r<BN, true, true>(x, w, scale, shift, res, y, M, K, N, relu, pscale, pshift, sub_w, sub_hw, st);
        return launch_pw_fwd_r<BN, true, false>(x, w, scale, shift, res, y, M, K, N, relu, pscale, pshift, sub_w, sub_hw, st);
    }
    if (res != nullptr)
        return launch_pw_fwd_r<BN, false, true>(x, w, scale, shift, res, y, M, K, N, relu, pscale, pshift, sub_w, sub_hw, st);
    return launch_pw_fwd_r<BN, false, false>(x, w, scale, shift, res, y, M, K, N, relu, pscale, pshift, sub_w, sub_hw, st);
}

}  // namespace

// Which output-channel tile BO a G3 = false call runs at.  Every tile gives the same bits (same MFMA sequence, same
// rounding points: only the split of pixels and output channels over workgroups differs), so this is a matter of speed
// alone.  0 = the table below, 1 = the narrow tiles (128, or 64 where K % 128) everywhere, 2 = the widest tile that
// divides K (512, 256) wherever one does.
static int g_pw_route_policy = 0;

// The table: (K, N), a range of M and the tile that won there.  A row is in it only where that tile's median beat the
// narrow tile's median by more than the narrow tile's own max - min over five alternating rounds, and it names the
// faster of the two wide tiles (tools/bench_pw_wide.py --only kernels at --batch 512, 256, 128 and 64:
// profiles/pw_wide_bench.json and pw_wide_bench_b{256,128,64}.json).  The bounds are the measured pixel counts
// (B x 28 x 28, B x 14 x 14, B x 7 x 7 at those batches), open above where the largest batch passed.  Next to the bytes,
// what decides is the round fit: a wide tile runs one workgroup per CU (256 slots), the narrow one two (512 slots) with
// 2 or 4 times the workgroups.  So the stage-3 conv3 gradient (K = 256) wins at 196 and 392 wide workgroups and loses at
// 784 (3.06 rounds pay for 4), and 512 loses to 256 once it leaves most CUs without a workgroup.  K = 256 with
// N <= 128 (stages 1 and 2, at the HBM limit already) never passed.
struct PwWideRow { int K, N, m_lo, m_hi, bo; };
static const PwWideRow kPwWide[] = {
    {512, 128, 200704, INT32_MAX, 512},    // layer2 conv1:        167 -> 152 us at B = 512; slower at B = 128
    {512, 256, 50176, INT32_MAX, 512},     // layer3.0 conv1:      280 -> 230 us at B = 512
    {256, 1024, 25088, 50176, 256},        // layer3 conv3:         65 -> 43 us at B = 128, 117 -> 106 at 256; 203 -> 208 at 512
    {1024, 256, 12544, INT32_MAX, 512},    // layer3 conv1:        139 -> 114 us at B = 512
    {1024, 512, 12544, INT32_MAX, 512},    // layer4.0 conv1:      236 -> 185 us at B = 512
    {512, 2048, 25088, INT32_MAX, 512},    // layer4 conv3:        257 -> 133 us at B = 512 (256: 151)
    {512, 2048, 12544, 25087, 256},        //                      123 -> 71 us at B = 256 (512: 89)
    {2048, 512, 6272, INT32_MAX, 512},     // layer4 conv1:        114 -> 97 us at B = 512
    {2048, 512, 3136, 6271, 256},
    {512, 1024, 25088, INT32_MAX, 512},    // layer3.0 downsample: 199 -> 173 us at B = 512
    {512, 1024, 12544, 25087, 256},
    {1024, 2048, 12544, INT32_MAX, 512},   // layer4.0 downsample: 203 -> 145 us at B = 512
    {1024, 2048, 3136, 12543, 256},
};

static int pw_bwd_tile(int M, int K, int N) {
    const int narrow = (K % 128 == 0) ? 128 : 64;
    if (K % 256 || g_pw_route_policy == 1) return narrow;
    if (g_pw_route_policy == 2) return (K % 512 == 0) ? 512 : 256;
    for (const PwWideRow& r : kPwWide)
        if (r.K == K && r.N == N && M >= r.m_lo && M <= r.m_hi) return r.bo;
    return narrow;
}

static int pw_bwd_check(const void* g, const void* y, const float* scale, const void* wt, void* gx, int M, int K, int N,
                        int relu, const void* xin, const float* pscale, const float* pshift, const void* g3, int sub_w,
                        int sub_hw) {
    if (!g || !scale || !wt || !gx || (relu && !y) || M <= 0 || K <= 0 || N <= 0 || (N % PW_BK) || (K % 64) || N > 2048)
        return ADIL_EINVAL;
    if (xin && (!pscale || !pshift)) return ADIL_EINVAL;
    if (g3 && (sub_w <= 0 || sub_hw <= 0 || sub_hw % sub_w || M % (4 * sub_hw))) return ADIL_EINVAL;
    return 0;
}

static int pw_bwd_run(int bo, const void* g, const void* g2, const void* y, const float* scale, const void* wt, void* gx,
                      void* gres, int M, int K, int N, int relu, const void* xin, const float* pscale, const float* pshift,
                      const void* g3, int sub_w, int sub_hw, hipStream_t st) {
    if (g3) {
        if (bo == 128)
            return launch_pw_bwd<128, true>(g, g2, y, scale, wt, gx, gres, M, K, N, relu, xin, pscale, pshift, g3, sub_w, sub_hw, st);
        return launch_pw_bwd<64, true>(g, g2, y, scale, wt, gx, gres, M, K, N, relu, xin, pscale, pshift, g3, sub_w, sub_hw, st);
    }
    if (bo == 512)
        return launch_pw_bwd<512, false, 8>(g, g2, y, scale, wt, gx, gres, M, K, N, relu, xin, pscale, pshift, nullptr, 0, 0, st);
    if (bo == 256)
        return launch_pw_bwd<256, false, 8>(g, g2, y, scale, wt, gx, gres, M, K, N, relu, xin, pscale, pshift, nullptr, 0, 0, st);
    if (bo == 128)
        return launch_pw_bwd<128, false>(g, g2, y, scale, wt, gx, gres, M, K, N, relu, xin, pscale, pshift, nullptr, 0, 0, st);
    return launch_pw_bwd<64, false>(g, g2, y, scale, wt, gx, gres, M, K, N, relu, xin, pscale, pshift, nullptr, 0, 0, st);
}

extern "C" int adil_pw_conv_bwd(const void* g, const void* g2, const void* y, const float* scale, const void* wt, void* gx,
                                void* gres, int M, int K, int N, int relu, const void* xin, const float* pscale,
                                const float* pshift, const void* g3, int sub_w, int sub_hw, void* stream) {
    ADIL_ENTER();
    const int rc = pw_bwd_check(g, y, scale, wt, gx, M, K, N, relu, xin, pscale, pshift, g3, sub_w, sub_hw);
    if (rc) return rc;
    const int bo = g3 ? ((K % 128 == 0) ? 128 : 64) : pw_bwd_tile(M, K, N);
    return pw_bwd_run(bo, g, g2, y, scale, wt, gx, gres, M, K, N, relu, xin, pscale, pshift, g3, sub_w, sub_hw, (hipStream_t)stream);
}

extern "C" int adil_pw_conv_bwd_tile(const void* g, const void* g2, const void* y, const float* scale, const void* wt,
                                     void* gx, void* gres, int M, int K, int N, int relu, const void* xin,
                                     const float* pscale, const float* pshift, const void* g3, int sub_w, int sub_hw,
                                     void* stream, int bo) {
    ADIL_ENTER();
    const int rc = pw_bwd_check(g, y, scale, wt, gx, M, K, N, relu, xin, pscale, pshift, g3, sub_w, sub_hw);
    if (rc) return rc;
    if ((bo != 64 && bo != 128 && bo != 256 && bo != 512) || K % bo || (bo >= 256 && g3)) return ADIL_EINVAL;
    return pw_bwd_run(bo, g, g2, y, scale, wt, gx, gres, M, K, N, relu, xin, pscale, pshift, g3, sub_w, sub_hw, (hipStream_t)stream);
}

extern "C" int adil_pw_route_policy(int policy) {
    const int prev = g_pw_route_policy;
    if (policy >= 0 && policy <= 2) g_pw_route_policy = policy;
    return prev;
}

// The forward tile BN under the same policy: 0 = the table below, 1 = the narrow tiles (128, or 64 where N % 128)
// everywhere, 2 = the widest tile that divides N (512, 256) wherever one does.  The table follows the rule of kPwWide:
// a row is in it only where the wide tile's median beat the narrow tile's median by more than the narrow tile's own
// max - min over five alternating rounds, it names the faster of the two wide tiles, and its M bounds are the measured
// pixel counts (tools/bench_pw_fwd.py at --batch 512, 256, 128 and 64: profiles/pw_fwd_bench.json and
// pw_fwd_bench_b{256,128,64}.json), from the smallest to the largest one that passed, open above where B = 512 did.
// Unlike the gradient, the forward narrow tile is not short of residents (3 - 4 workgroups per CU, 600 - 790 TFLOP/s on
// the long-K shapes at B = 512), and a wide tile is ONE workgroup per CU whose load, MFMA and store phases overlap with
// nobody's: it wins where the narrow grid no longer fills the CUs (small M) or K is long enough to hide its ends
// (K = 2048), and loses 10 - 35 % on every conv3 shape (K <= 512, N = 4 K) at B >= 256.
struct PwFwdWideRow { int K, N, m_lo, m_hi, bn; };
static const PwFwdWideRow kPwFwdWide[] = {
    {2048, 512, 12544, INT32_MAX, 256},    // layer4 conv1:        84 -> 77 us at B = 512 (512: 85), 47 -> 39 at 256; 34 -> 37 at 128
    {1024, 256, 25088, 50176, 256},        // layer3 conv1:        48 -> 46 us at B = 256, 29 -> 25 at 128; 81 -> 95 at 512
    {1024, 512, 12544, 12544, 256},        // layer4.0 conv1:      29 -> 24 us at B = 64; 49 -> 47 at 128 is inside the spread
    {1024, 2048, 3136, 3136, 256},         // layer4.0 downsample: 29 -> 25 us at B = 64
    {512, 1024, 12544, 12544, 512},        // layer3.0 downsample: 29.8 -> 29.2 us at B = 64 (256: 30.7)
    {512, 2048, 6272, 6272, 512},          // layer4 conv3:        36.4 -> 35.8 us at B = 128 (256: 36.9)
    {512, 2048, 3136, 3136, 256},          //                      21.5 -> 20.5 us at B = 64 (512: 33.8)
};

static int pw_fwd_tile(int M, int K, int N) {
    const int narrow = (N % 128 == 0) ? 128 : 64;
    if (N % 256 || g_pw_route_policy == 1) return narrow;
    if (g_pw_route_policy == 2) return (N % 512 == 0) ? 512 : 256;
    for (const PwFwdWideRow& r : kPwFwdWide)
        if (r.K == K && r.N == N && M >= r.m_lo && M <= r.m_hi) return r.bn;
    return narrow;
}

static int pw_fwd_check(const void* x, const void* w, const float* scale, const float* shift, void* y, int M, int K, int N,
                        const float* pscale, const float* pshift, int sub_w, int sub_hw) {
    if (!x || !w || !scale || !shift || !y || M <= 0 || K <= 0 || N <= 0 || (K % PW_BK) || (N % 64)) return ADIL_EINVAL;
    if ((pscale != nullptr) != (pshift != nullptr) || (pscale && K > PW_PK)) return ADIL_EINVAL;
    if (sub_w < 0 || (sub_w > 0 && (sub_hw <= 0 || sub_hw % sub_w || M % sub_hw))) return ADIL_EINVAL;
    return 0;
}

static int pw_fwd_run(int bn, const void* x, const void* w, const float* scale, const float* shift, const void* res, void* y,
                      int M, int K, int N, int relu, const float* pscale, const float* pshift, int sub_w, int sub_hw,
                      hipStream_t st) {
    if (bn == 512) return launch_pw_fwd<512>(x, w, scale, shift, res, y, M, K, N, relu, pscale, pshift, sub_w, sub_hw, st);
    if (bn == 256) return launch_pw_fwd<256>(x, w, scale, shift, res, y, M, K, N, relu, pscale, pshift, sub_w, sub_hw, st);
    if (bn == 128) return launch_pw_fwd<128>(x, w, scale, shift, res, y, M, K, N, relu, pscale, pshift, sub_w, sub_hw, st);
    return launch_pw_fwd<64>(x, w, scale, shift, res, y, M, K, N, relu, pscale, pshift, sub_w, sub_hw, st);
}

extern "C" int adil_pw_conv_fwd(const void* x, const void* w, const float* scale, const float* shift, const void* res,
                                void* y, int M, int K, int N, int relu, const float* pscale, const float* pshift,
                                int sub_w, int sub_hw, void* stream) {
    ADIL_ENTER();
    const int rc = pw_fwd_check(x, w, scale, shift, y, M, K, N, pscale, pshift, sub_w, sub_hw);
    if (rc) return rc;
    return pw_fwd_run(pw_fwd_tile(M, K, N), x, w, scale, shift, res, y, M, K, N, relu, pscale, pshift, sub_w, sub_hw,
                      (hipStream_t)stream);
}

extern "C" int adil_pw_conv_fwd_tile(const void* x, const void* w, const float* scale, const float* shift, const void* res,
                                     void* y, int M, int K, int N, int relu, const float* pscale, const float* pshift,
                                     int sub_w, int sub_hw, void* stream, int bn) {
    ADIL_ENTER();
    const int rc = pw_fwd_check(x, w, scale, shift, y, M, K, N, pscale, pshift, sub_w, sub_hw);
    if (rc) return rc;
    if ((bn != 64 && bn != 128 && bn != 256 && bn != 512) || N % bn) return ADIL_EINVAL;
    return pw_fwd_run(bn, x, w, scale, shift, res, y, M, K, N, relu, pscale, pshift, sub_w, sub_hw, (hipStream_t)stream);
}

// =========================================================================================================== //
// Residual join of two consecutive bottlenecks of one stage as ONE kernel: conv3 of block i-1 (width WD -> C = 4 WD,
// bn2 + ReLU prologue, bn3 + residual + ReLU epilogue) and conv1 of block i (C -> WD, bn1 + ReLU), or the input
// gradient of the pair.  The C-channel tensor between the two GEMMs (`out` forward, the conv1 input gradient `t`
// backward) never goes through HBM as an operand:
//   forward   X0 = relu(h2raw * pscale2 + pshift2)              [128 px][WD], staged once
//             per 64-channel chunk j of C:  A_j = X0 . W3[j]^T -> bn3 + res + ReLU -> out[:, j] (stored, and kept in
//             LDS as the K chunk j of GEMM 2)                    B += out[:, j] . W1[:, j]^T
//             h1 = relu(B * scale1 + shift1)
//   backward  X0 = (g_h1 * [h1 > 0] * scale1)                   per chunk j:  t_j = bf16(X0 . Wt1[j]^T),
//             v = t_j + g_out[:, j],  gres[:, j] = v * [out > 0],  G += (v * scale3 * [out > 0]) . Wt3[:, j]^T
//             gx = G * [h2raw * pscale2 + pshift2 > 0] * pscale2
// Every value is rounded where pw_conv_fwd / pw_conv_bwd round it and every accumulator sees the same MFMA sequence
// (chunk j of C is the 64-wide K chunk j of the second GEMM), so the results are bitwise those of the two-kernel route.
// Workgroup = 128 pixels (4 waves x 32), MFMA roles as in pw_conv_*.  X0 rows, the mid chunk and the output
// transposes are private to the wave that owns the pixels; only the two weight chunks are shared (2 barriers / chunk).
// LDS: X0 [128][WD+8] | Wa chunk [64][WD+8] | Wb chunk [WD][72] | mid [128][72]:  54 KB at WD = 64 (2 workgroups per
// CU), 87 KB at WD = 128 (1).  The epilogue inputs of chunk j+1 (residual / g_out, out) are loaded under chunk j.
// =========================================================================================================== //
namespace {

struct JoinArgs {
    const bf16_t* x0;       // fwd: h2raw [M][WD]         bwd: g_h1 [M][WD]
    const bf16_t* y0;       //                            bwd: h1 [M][WD] (ReLU mask)
    const float* s0;        // fwd: pscale2 [WD]          bwd: scale1 [WD]
    const float* b0;        // fwd: pshift2 [WD]
    const bf16_t* wa;       // [C][WD]  fwd: conv3 weight, bwd: conv1 weight transposed
    const float* sa;        // [C]      scale3
    const float* ba;        // [C]      fwd: shift3
    const bf16_t* ra;       // [M][C]   fwd: residual     bwd: g_out
    const bf16_t* ya;       // [M][C]                     bwd: out (ReLU mask)
    bf16_t* oa;             // [M][C]   fwd: out          bwd: gres
    const bf16_t* wb;       // [WD][C]  fwd: conv1 weight, bwd: conv3 weight transposed
    const float* sb;        // [WD]     fwd: scale1       bwd: pscale2
    const float* bb;        // [WD]     fwd: shift1       bwd: pshift2
    const bf16_t* xin;      // [M][WD]                    bwd: h2raw
    bf16_t* ob;             // [M][WD]  fwd: h1           bwd: gx
    int M, C;
};

template <int WD, bool BWD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WD == 64 ? 2 : 1))) void pw_join_kernel(JoinArgs p) {
    constexpr int XS = WD + 8;                           // X0 / output-transpose row stride (elements): odd x 16 B
    constexpr int CTB = WD / 32;                         // second GEMM: channel tiles per wave
    constexpr int X0C = WD / 16;                         // 16-byte chunks of a wave's 32 X0 rows per lane
    constexpr int WAC = WD / 32;                         // ... of a Wa chunk [64][WD] per thread
    constexpr int WBC = WD / 32;                         // ... of a Wb chunk [WD][64] per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sx0 = reinterpret_cast<bf16_t*>(smem_raw);   // [128][XS]
    bf16_t* swa = sx0 + PW_BM * XS;                      // [64][XS]
    bf16_t* swb = swa + 64 * XS;                         // [WD][PW_LS]
    bf16_t* smid = swb + WD * PW_LS;                     // [128][PW_LS]
    __shared__ __attribute__((aligned(16))) float stab[2 * 4 * 128];   // scale3 | shift3 (C <= 512)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int M = p.M, C = p.C, nch = C / 64;
    const int m0 = blockIdx.x * PW_BM;
    const int m = m0 + w * 32 + c;                       // this lane's pixel in the epilogues
    const size_t mc = (size_t)(m < M ? m : M - 1);
    bf16_t* sxw = sx0 + w * 32 * XS;                     // this wave's X0 rows (later: its output transpose)
    bf16_t* smw = smid + w * 32 * PW_LS;                 // this wave's mid rows

    u32x4 ar[WAC], br[WBC];
    auto load_w = [&](int j) {
#pragma unroll
        for (int i = 0; i < WAC; ++i) {
            const int id = tid + 256 * i, row = id / (WD / 8), ch = id % (WD / 8);
            ar[i] = *reinterpret_cast<const u32x4*>(p.wa + (size_t)(64 * j + row) * WD + ch * 8);
        }
#pragma unroll
        for (int i = 0; i < WBC; ++i) {
            const int id = tid + 256 * i, row = id >> 3, ch = id & 7;
            br[i] = *reinterpret_cast<const u32x4*>(p.wb + (size_t)row * C + 64 * j + ch * 8);
        }
    };
    auto store_w = [&]() {
#pragma unroll
        for (int i = 0; i < WAC; ++i) {
            const int id = tid + 256 * i, row = id / (WD / 8), ch = id % (WD / 8);
            *reinterpret_cast<u32x4*>(swa + row * XS + ch * 8) = ar[i];
        }
#pragma unroll
        for (int i = 0; i < WBC; ++i) {
            const int id = tid + 256 * i, row = id >> 3, ch = id & 7;
            *reinterpret_cast<u32x4*>(swb + row * PW_LS + ch * 8) = br[i];
        }
    };
    // epilogue inputs of a chunk in the accumulator layout: lane = pixel m, quad q of tile ct = channels 32ct+8q+4h..+3
    u32x2 er[2][4], ey[BWD ? 2 : 1][4];
    auto load_e = [&](int j) {
        const bf16_t* rp = p.ra + mc * C + 64 * j + 4 * h;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int q = 0; q < 4; ++q) er[ct][q] = *reinterpret_cast<const u32x2*>(rp + 32 * ct + 8 * q);
        if (BWD) {
            const bf16_t* yp = p.ya + mc * C + 64 * j + 4 * h;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int q = 0; q < 4; ++q) ey[BWD ? ct : 0][q] = *reinterpret_cast<const u32x2*>(yp + 32 * ct + 8 * q);
        }
    };

    // X0: this wave's 32 pixels, transformed on the way to LDS exactly as pw_conv_fwd's prologue (forward) or
    // pw_conv_bwd's operand path without g2 (backward) transforms them
    {
        u32x4 xr[X0C], yr[BWD ? X0C : 1];
#pragma unroll
        for (int i = 0; i < X0C; ++i) {
            const int id = lane + 64 * i, r = id / (WD / 8), ch = id % (WD / 8);
            const int mm = m0 + w * 32 + r;
            const size_t at = (size_t)(mm < M ? mm : M - 1) * WD + ch * 8;
            xr[i] = *reinterpret_cast<const u32x4*>(p.x0 + at);
            if (BWD) yr[BWD ? i : 0] = *reinterpret_cast<const u32x4*>(p.y0 + at);
        }
        load_w(0);
        load_e(0);
        if (tid < C / 4) *reinterpret_cast<float4*>(stab + 4 * tid) = *reinterpret_cast<const float4*>(p.sa + 4 * tid);
        if (!BWD && tid < C / 4) *reinterpret_cast<float4*>(stab + C + 4 * tid) = *reinterpret_cast<const float4*>(p.ba + 4 * tid);
#pragma unroll
        for (int i = 0; i < X0C; ++i) {
            const int id = lane + 64 * i, r = id / (WD / 8), ch = id % (WD / 8);
            const f32x2* ps = reinterpret_cast<const f32x2*>(p.s0 + ch * 8);
            u32x4 t = xr[i];
            if (BWD) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x2 v = bf2_to_f32x2(t[j]);
                    t[j] = f32x2_to_bf2(v * ps[j]) & pos_mask_bf2(yr[BWD ? i : 0][j]);
                }
            } else {
                const f32x2* pb = reinterpret_cast<const f32x2*>(p.b0 + ch * 8);
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = relu_bf2(f32x2_to_bf2(bf2_to_f32x2(t[j]) * ps[j] + pb[j]));
            }
            *reinterpret_cast<u32x4*>(sxw + r * XS + ch * 8) = t;
        }
    }
    store_w();
    __syncthreads();

    f32x16 accb[CTB];
#pragma unroll
    for (int ct = 0; ct < CTB; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) accb[ct][r] = 0.0f;
    const bf16_t* bx = sxw + c * XS + 8 * h;
    const bf16_t* bm = smw + c * PW_LS + 8 * h;
    for (int j = 0; j < nch; ++j) {
        if (j + 1 < nch) load_w(j + 1);
        // GEMM 1: 32 px x 64 channels of chunk j per wave, K = WD in the k order of the two-kernel route
        f32x16 acca[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acca[ct][r] = 0.0f;
        const bf16_t* ba = swa + c * XS + 8 * h;
#pragma unroll
        for (int ks = 0; ks < WD / 16; ++ks) {
            const bf16x8 b = lds8(bx + 16 * ks);
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) mma16(acca[ct], lds8(ba + ct * 32 * XS + 16 * ks), b);
        }
        // chunk epilogue on the accumulators -> this wave's mid rows
        u32x2 gz[BWD ? 2 : 1][4];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co = 32 * ct + 8 * q + 4 * h;
                const f32x2* sc = reinterpret_cast<const f32x2*>(stab + 64 * j + co);
                u32x2 t;
                if (BWD) {
                    u32x2 z;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const f32x2 v = bf2_to_f32x2(pack2_bf16(acca[ct][4 * q + 2 * e], acca[ct][4 * q + 2 * e + 1])) +
                                        bf2_to_f32x2(er[ct][q][e]);
                        const unsigned mk = pos_mask_bf2(ey[BWD ? ct : 0][q][e]);
                        t[e] = f32x2_to_bf2(v) & mk;
                        z[e] = f32x2_to_bf2(v * sc[e]) & mk;
                    }
                    gz[BWD ? ct : 0][q] = z;
                } else {
                    const f32x2* sh = reinterpret_cast<const f32x2*>(stab + C + 64 * j + co);
                    f32x2 v0 = f32x2{acca[ct][4 * q], acca[ct][4 * q + 1]} * sc[0] + sh[0];
                    f32x2 v1 = f32x2{acca[ct][4 * q + 2], acca[ct][4 * q + 3]} * sc[1] + sh[1];
                    v0 += bf2_to_f32x2(er[ct][q][0]);
                    v1 += bf2_to_f32x2(er[ct][q][1]);
                    t[0] = relu_bf2(f32x2_to_bf2(v0));
                    t[1] = relu_bf2(f32x2_to_bf2(v1));
                }
                *reinterpret_cast<u32x2*>(smw + c * PW_LS + co) = t;
            }
        }
        if (j + 1 < nch) load_e(j + 1);                 // flies under GEMM 2 and the next chunk's GEMM 1
        // out (forward) / gres (backward) chunk: 16-byte stores from the transposed rows
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int id = lane + 64 * i, px = id >> 3, ch = id & 7;
            const u32x4 t = *reinterpret_cast<const u32x4*>(smw + px * PW_LS + ch * 8);
            const int mm = m0 + w * 32 + px;
            if (mm < M) *reinterpret_cast<u32x4*>(p.oa + (size_t)mm * C + 64 * j + ch * 8) = t;
        }
        if (BWD) {                                      // the operand of GEMM 2 is the scaled chunk, not gres
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<u32x2*>(smw + c * PW_LS + 32 * ct + 8 * q + 4 * h) = gz[BWD ? ct : 0][q];
        }
        // GEMM 2: chunk j is the 64-wide K chunk j
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 b = lds8(bm + 16 * ks);
#pragma unroll
            for (int ct = 0; ct < CTB; ++ct) mma16(accb[ct], lds8(swb + (ct * 32 + c) * PW_LS + 8 * h + 16 * ks), b);
        }
        lds_barrier();                                  // every wave is done with this chunk's weights
        if (j + 1 < nch) {
            store_w();
            lds_barrier();
        }
    }
    // final epilogue through this wave's X0 rows (nobody else reads them) -> 16-byte stores of h1 / gx
#pragma unroll
    for (int ct = 0; ct < CTB; ++ct) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int co = 32 * ct + 8 * q + 4 * h;
            u32x2 t;
            if (BWD) {
                t[0] = pack2_bf16(accb[ct][4 * q], accb[ct][4 * q + 1]);
                t[1] = pack2_bf16(accb[ct][4 * q + 2], accb[ct][4 * q + 3]);
            } else {
                const f32x2* sc = reinterpret_cast<const f32x2*>(p.sb + co);
                const f32x2* sh = reinterpret_cast<const f32x2*>(p.bb + co);
                f32x2 v0 = f32x2{accb[ct][4 * q], accb[ct][4 * q + 1]} * sc[0] + sh[0];
                f32x2 v1 = f32x2{accb[ct][4 * q + 2], accb[ct][4 * q + 3]} * sc[1] + sh[1];
                t[0] = relu_bf2(f32x2_to_bf2(v0));
                t[1] = relu_bf2(f32x2_to_bf2(v1));
            }
            *reinterpret_cast<u32x2*>(sxw + c * XS + co) = t;
        }
    }
    constexpr int CPP = WD / 8;
#pragma unroll
    for (int i = 0; i < 32 * CPP / 64; ++i) {
        const int id = lane + 64 * i, px = id / CPP, ch = id - px * CPP;
        u32x4 t = *reinterpret_cast<const u32x4*>(sxw + px * XS + ch * 8);
        const int mm = m0 + w * 32 + px;
        if (mm < M) {
            if (BWD) {
                float v[8], xv[8];
                unpack8(t, v);
                unpack8(*reinterpret_cast<const u32x4*>(p.xin + (size_t)mm * WD + ch * 8), xv);
                const float4 a0 = *reinterpret_cast<const float4*>(p.sb + ch * 8);
                const float4 a1 = *reinterpret_cast<const float4*>(p.sb + ch * 8 + 4);
                const float4 b0 = *reinterpret_cast<const float4*>(p.bb + ch * 8);
                const float4 b1 = *reinterpret_cast<const float4*>(p.bb + ch * 8 + 4);
                const float ps[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                const float pb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (xv[e] * ps[e] + pb[e] > 0.0f) ? v[e] * ps[e] : 0.0f;
                t = pack8(v);
            }
            *reinterpret_cast<u32x4*>(p.ob + (size_t)mm * WD + ch * 8) = t;
        }
    }
}

template <int WD, bool BWD>
int launch_pw_join(const JoinArgs& a, hipStream_t st) {
    const size_t lds = ((size_t)(PW_BM + 64) * (WD + 8) + (size_t)(WD + PW_BM) * PW_LS) * sizeof(bf16_t);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)pw_join_kernel<WD, BWD>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((pw_join_kernel<WD, BWD>), dim3((unsigned)((a.M + PW_BM - 1) / PW_BM)), dim3(256), lds, st, a);
    ADIL_CHECK_LAUNCH();
    return 0;
}

template <bool BWD>
int launch_pw_join_w(const JoinArgs& a, int W, hipStream_t st) {
    if (W == 64) return launch_pw_join<64, BWD>(a, st);
    return launch_pw_join<128, BWD>(a, st);
}

}  // namespace

extern "C" int adil_pw_join_fwd(const void* h2raw, const float* pscale2, const float* pshift2, const void* w3,
                                const float* scale3, const float* shift3, const void* res, void* out, const void* w1,
                                const float* scale1, const float* shift1, void* h1, int M, int W, int C, void* stream) {
    ADIL_ENTER();
    if (!h2raw || !pscale2 || !pshift2 || !w3 || !scale3 || !shift3 || !res || !out || !w1 || !scale1 || !shift1 || !h1 ||
        M <= 0 || (W != 64 && W != 128) || C != 4 * W)
        return ADIL_EINVAL;
    const JoinArgs a = {(const bf16_t*)h2raw, nullptr, pscale2, pshift2, (const bf16_t*)w3, scale3, shift3,
                        (const bf16_t*)res, nullptr, (bf16_t*)out, (const bf16_t*)w1, scale1, shift1, nullptr, (bf16_t*)h1,
                        M, C};
    return launch_pw_join_w<false>(a, W, (hipStream_t)stream);
}

extern "C" int adil_pw_join_bwd(const void* g_h1, const void* h1, const float* scale1, const void* wt1, const void* g_out,
                                const void* out, const float* scale3, void* gres, const void* wt3, const void* h2raw,
                                const float* pscale2, const float* pshift2, void* gx, int M, int W, int C, void* stream) {
    ADIL_ENTER();
    if (!g_h1 || !h1 || !scale1 || !wt1 || !g_out || !out || !scale3 || !gres || !wt3 || !h2raw || !pscale2 || !pshift2 ||
        !gx || M <= 0 || (W != 64 && W != 128) || C != 4 * W)
        return ADIL_EINVAL;
    const JoinArgs a = {(const bf16_t*)g_h1, (const bf16_t*)h1, scale1, nullptr, (const bf16_t*)wt1, scale3, nullptr,
                        (const bf16_t*)g_out, (const bf16_t*)out, (bf16_t*)gres, (const bf16_t*)wt3, pscale2, pshift2,
                        (const bf16_t*)h2raw, (bf16_t*)gx, M, C};
    return launch_pw_join_w<true>(a, W, (hipStream_t)stream);
}

// =========================================================================================================== //
// 3x3 / stride 2 / pad 1 convolution of the frozen ResNet (conv2 of the first bottleneck of stages 2-4; conv1 of the
// same BasicBlocks), NHWC bf16, raw output, forward AND input gradient, even H and W.  Both are a sum of tap-GEMMs
// over rows r = (b, i, j) of the OH x OW = H/2 x W/2 grid:
//   forward    y[r][n]  = sum_{kh,kw,c} x[(b, 2i-1+kh, 2j-1+kw)][c] * wp[n][kh*3+kw][c]      (9 taps; only kh = 0 at
//              i = 0 and kw = 0 at j = 0 leave the image: H, W even).  Centre tap = input pixel 4r - 2j.
//   gradient   input pixels fall into four parity classes (ph, pw) = (h & 1, w & 1); pixel (2i+ph, 2j+pw) receives
//              gx[(b, 2i+ph, 2j+pw)][c] = sum_{kh in KH(ph), kw in KW(pw), n} g[(b, i + [kh = 0], j + [kw = 0])][n] * wpb[c][kh*3+kw][n]
//              with KH(0) = {1}, KH(1) = {0, 2} (same for kw): 1 / 2 / 2 / 4 live taps, 9 tap-GEMMs per 2x2 block — the
//              forward's FLOP count; no zero-upsampled g exists anywhere.  A workgroup owns 128 rows r and runs the four
//              classes one after the other (every workgroup does the same 9 tap-GEMMs; the g rows stay in L2), writing
//              input pixels 4r - 2j + ph*W + pw class by class.
// One kernel does both: per (64-channel chunk, tap) the 128 source rows of the tap are gathered from global memory
// (rows of a tap that leaves the image are zeroed on the way to LDS) next to the [BN][64] weight tile; both tiles are
// double buffered in LDS with the next three pairs in registers or in flight (across class boundaries too), one barrier
// per tap, 16 MFMAs per wave on 64 px x 64 (32) channel wave tiles as in conv3x3_kernel; a finished class leaves through
// the idle buffer.  No zero-fill launch, no atomics: bitwise reproducible.
// =========================================================================================================== //
namespace {

#define S2_BM 128
#define C3_LS 72                       // LDS row pitch in bf16 (64 channels + 8), as in conv3x3_kernel

// The main loop is conv3x3_kernel's (adil_conv3x3.hip) as far as it has the same shape (the taps stay run-time values: the gradient's classes
// have 4 / 2 / 2 / 1 of them): per-thread byte offsets computed once (weights 32-bit on a uniform base, source rows plus a
// uniform tap offset); at BN = 64 two fragment register sets and the barrier between the MFMAs of ks = 2 and ks = 3, a
// finished class then leaving through the buffer whose tile it has just multiplied; at BN = 128 the second fragment set
// would spill, so a tap reads its fragments in front of its MFMAs and the barrier closes it.
template <int BN, bool BWD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void conv3x3_s2_kernel(
    const bf16_t* __restrict__ src, const bf16_t* __restrict__ wp, bf16_t* __restrict__ dst, int M, int OH, int OW, int K,
    int NO, int MT, int NT) {
    constexpr int CTW = BN / 64;                         // channel tiles per wave (2 x 2 waves: 64 px x BN/2 channels)
    constexpr int XCH = S2_BM * 8 / 256;                 // 16-byte chunks of a source tile per thread (4)
    constexpr int WCH = BN * 8 / 256;                    // ... of a weight tile
    constexpr int OS = BN + 8;
    constexpr int PAIR = (S2_BM + BN) * C3_LS;           // one buffer: source tile [128][C3_LS] | weight tile [BN][C3_LS]
    constexpr int NCLS = BWD ? 4 : 1;
    constexpr bool PIPE = BN == 64;                      // at BN = 128 the second fragment set spills
    static_assert(S2_BM * OS <= PAIR, "the output transpose goes through one idle buffer");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sb = reinterpret_cast<bf16_t*>(smem_raw);    // [2][PAIR]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int wpx = w & 1, wch = w >> 1;
    int mt, nt;
    if ((MT & 7) == 0) {                                 // the workgroups of one row tile go to ONE XCD (see pw_conv_fwd_kernel)
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        nt = j % NT;
        mt = (j / NT) * 8 + xcd;
    } else {
        nt = blockIdx.x % NT;
        mt = blockIdx.x / NT;
    }
    const int m0 = mt * S2_BM, n0 = nt * BN;
    const int nci = K >> 6;
    const int nit = nci * 9;                             // forward: 9 taps; gradient: 4 + 2 + 2 + 1 taps of the four classes
    // gradient classes in the order (ph, pw) = (1,1) (1,0) (0,1) (0,0); taps per direction
    auto cls_ph = [](int cls) { return BWD ? (cls < 2 ? 1 : 0) : 0; };
    auto cls_pw = [](int cls) { return BWD ? ((cls & 1) ? 0 : 1) : 0; };

    // the rows this thread stages: centre source row and which of its taps stay inside the image
    int ctr[XCH];
    unsigned flg[XCH];                                   // bit 0: row < M, bit 1: kh = 0 is inside, bit 2: kw = 0 is inside
#pragma unroll
    for (int i = 0; i < XCH; ++i) {
        const int r = m0 + (tid >> 3) + 32 * i;
        const int rc = r < M ? r : M - 1;
        const int j = rc % OW, ii = (rc / OW) % OH;
        ctr[i] = BWD ? rc : 4 * rc - 2 * j;
        const bool okh = BWD ? (ii + 1 < OH) : (ii > 0), okw = BWD ? (j + 1 < OW) : (j > 0);
        flg[i] = (r < M ? 1u : 0u) | (okh ? 2u : 0u) | (okw ? 4u : 0u);
    }
    // a (source, weight) tile pair on its way to LDS; three are in flight: tile it+3 is requested while tile it is
    // multiplied (an L2 round trip is several times the 16 MFMAs of one tap, see conv3x3_kernel)
    struct Tile {
        u32x4 x[XCH], w[WCH];
        unsigned ok;                                     // bit i: chunk i of x is real data (else a tap outside the image)
    };
    // (class, channel chunk, tap row, tap column) of the NEXT load_tiles call: tiles are requested in the order they
    // are multiplied, class after class
    int lcls = 0, lcc = 0, la = 0, lb = 0;
    int lph = cls_ph(0), lpw = cls_pw(0), lnth = BWD ? 1 + lph : 3, lntw = BWD ? 1 + lpw : 3;
    // byte offsets, once.  Source: this thread's centre rows; weights: 32 bits (the pack is below 2^31 elements).
    size_t sq[XCH];
#pragma unroll
    for (int i = 0; i < XCH; ++i) sq[i] = ((size_t)ctr[i] * K + (tid & 7) * 8) * sizeof(bf16_t);
    const unsigned wq = (((unsigned)(n0 + (tid >> 3)) * 9u) * (unsigned)K + (unsigned)(tid & 7) * 8u) * 2u;
    const size_t wrow = (size_t)32 * 9 * K;                  // elements between a thread's weight rows (uniform)
    auto load_tiles = [&](Tile& t) {
        const int kh = BWD ? (lph ? 2 * la : 1) : la, kw = BWD ? (lpw ? 2 * lb : 1) : lb;
        const int off = BWD ? (kh == 0 ? OW : 0) + (kw == 0 ? 1 : 0) : (kh - 1) * 2 * OW + (kw - 1);
        const unsigned need = 1u | (kh == 0 ? 2u : 0u) | (kw == 0 ? 4u : 0u);
        unsigned okm = 0;
        const char* sbase = reinterpret_cast<const char*>(src + lcc * 64);
        const long long toff = (long long)off * K * (long long)sizeof(bf16_t);   // uniform
#pragma unroll
        for (int i = 0; i < XCH; ++i) {
            const bool ok = (flg[i] & need) == need;
            okm |= ok ? (1u << i) : 0u;
            t.x[i] = *reinterpret_cast<const u32x4*>(sbase + sq[i] + (ok ? toff : 0LL));   // always a valid address
        }
        const bf16_t* wbase = wp + (kh * 3 + kw) * K + lcc * 64;
#pragma unroll
        for (int i = 0; i < WCH; ++i)
            t.w[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(wbase + i * wrow) + wq);
        t.ok = okm;
        if (++lb == lntw) {
            lb = 0;
            if (++la == lnth) {
                la = 0;
                if (++lcc == nci && lcls + 1 < NCLS) {
                    lcc = 0;
                    ++lcls;
                    lph = cls_ph(lcls);
                    lpw = cls_pw(lcls);
                    lnth = 1 + lph;
                    lntw = 1 + lpw;
                }
            }
        }
    };
    auto store_tiles = [&](int buf, const Tile& t) {
        bf16_t* sx = sb + buf * PAIR;
        bf16_t* sw = sx + S2_BM * C3_LS;
#pragma unroll
        for (int i = 0; i < XCH; ++i) {
            const int row = (tid >> 3) + 32 * i, ch = tid & 7;
            u32x4 v = t.x[i];
            const bool ok = (t.ok >> i) & 1u;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ok ? v[j] : 0u;
            *reinterpret_cast<u32x4*>(sx + row * C3_LS + ch * 8) = v;
        }
#pragma unroll
        for (int i = 0; i < WCH; ++i) {
            const int q = tid + 256 * i, row = q >> 3, ch = q & 7;
            *reinterpret_cast<u32x4*>(sw + row * C3_LS + ch * 8) = t.w[i];
        }
    };

    f32x16 acc[2][CTW];
    auto zero_acc = [&]() {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[p][ct][r] = 0.0f;
    };
    zero_acc();
    // a finished class (the forward's only one): transpose through the idle buffer (all waves share one [128][OS]
    // tile), 16-byte NHWC stores.  The tiles of the next class stay in flight in registers meanwhile.
    auto finish_class = [&](int cls, bf16_t* so) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int pl = wpx * 64 + p * 32 + c;
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    u32x2 t;
                    t[0] = pack2_bf16(acc[p][ct][4 * q], acc[p][ct][4 * q + 1]);
                    t[1] = pack2_bf16(acc[p][ct][4 * q + 2], acc[p][ct][4 * q + 3]);
                    *reinterpret_cast<u32x2*>(so + pl * OS + (wch * CTW + ct) * 32 + 8 * q + 4 * h) = t;
                }
            }
        }
        lds_barrier();
        const int ph = cls_ph(cls), pw = cls_pw(cls);
        constexpr int CPP = BN / 8;
#pragma unroll
        for (int i = 0; i < S2_BM * CPP / 256; ++i) {
            const int id = tid + 256 * i, px = id / CPP, ch = id - px * CPP;
            const int r = m0 + px;
            if (r < M) {
                const size_t drow = BWD ? (size_t)(4 * r - 2 * (r % OW) + ph * 2 * OW + pw) : (size_t)r;
                *reinterpret_cast<u32x4*>(dst + drow * NO + n0 + ch * 8) = *reinterpret_cast<const u32x4*>(so + px * OS + ch * 8);
            }
        }
        lds_barrier();                                   // the buffer is free for the next tile
        zero_acc();
    };

    int ccls = 0;                                        // the class being multiplied and the taps it has left
    int crem = nci * (BWD ? 4 : 9);
    [[maybe_unused]] auto tap_body = [&](int it, Tile& tfree, const Tile& tnext) {
        // on entry: LDS buffer it & 1 holds tile it, tnext holds tile it+1, the third register set tile it+2 (in
        // flight), tfree's tile is already in LDS
        const int buf = it & 1;
        if (it + 3 < nit) load_tiles(tfree);
        const bf16_t* bx = sb + buf * PAIR + (wpx * 64 + c) * C3_LS + 8 * h;
        const bf16_t* bw = sb + buf * PAIR + (S2_BM + wch * CTW * 32 + c) * C3_LS + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 b0 = lds8(bx + 16 * ks);
            const bf16x8 b1 = lds8(bx + 32 * C3_LS + 16 * ks);
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct) {
                const bf16x8 a = lds8(bw + ct * 32 * C3_LS + 16 * ks);
                mma16(acc[0][ct], a, b0);
                mma16(acc[1][ct], a, b1);
            }
        }
        // the other buffer was last read before the previous barrier: it takes the class's output transpose, then tile it+1
        if (--crem == 0) {                               // uniform: every wave meets the same barriers
            finish_class(ccls, sb + (buf ^ 1) * PAIR);
            ++ccls;
            crem = nci * (1 + cls_ph(ccls)) * (1 + cls_pw(ccls));
        }
        if (it + 1 < nit) store_tiles(buf ^ 1, tnext);
        lds_barrier();
    };

    // PIPE: fa holds the fragments of ks 0 and 2, fb those of ks 1 and 3; the reads of ks + 1 fly under the MFMAs of ks
    struct Frag {
        bf16x8 b0, b1, a[CTW];
    };
    auto read_frag = [&](Frag& f, int buf, int ks) {
        const bf16_t* bx = sb + buf * PAIR + (wpx * 64 + c) * C3_LS + 8 * h;
        const bf16_t* bw = sb + buf * PAIR + (S2_BM + wch * CTW * 32 + c) * C3_LS + 8 * h;
        f.b0 = lds8(bx + 16 * ks);
        f.b1 = lds8(bx + 32 * C3_LS + 16 * ks);
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
    Frag fa, fb;
    [[maybe_unused]] auto tap_body0 = [&](int it, Tile& tfree, const Tile& tnext) {
        // on entry: as tap_body, and fa holds this tile's ks = 0 fragments (in flight).  The other buffer was last read
        // before the previous barrier: tile it+1 goes there first, and the barrier comes once every wave has issued
        // its last reads of this tile, under the MFMAs of ks = 3
        const int buf = it & 1;
        read_frag(fb, buf, 1);
        if (it + 1 < nit) store_tiles(buf ^ 1, tnext);
        if (it + 3 < nit) load_tiles(tfree);
        __builtin_amdgcn_sched_barrier(0);
        mma_frag(fa);
        __builtin_amdgcn_sched_barrier(0);
        read_frag(fa, buf, 2);
        __builtin_amdgcn_sched_barrier(0);
        mma_frag(fb);
        __builtin_amdgcn_sched_barrier(0);
        read_frag(fb, buf, 3);
        __builtin_amdgcn_sched_barrier(0);
        mma_frag(fa);
        __builtin_amdgcn_sched_barrier(0);
        lds_barrier();
        if (it + 1 < nit) read_frag(fa, buf ^ 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        mma_frag(fb);
        __builtin_amdgcn_sched_barrier(0);
        // every wave read this tile before the barrier: its buffer takes the class's output transpose (tile it+2 goes
        // there only in the next tap, behind finish_class's own barriers)
        if (--crem == 0) {                               // uniform: every wave meets the same barriers
            finish_class(ccls, sb + buf * PAIR);
            ++ccls;
            crem = nci * (1 + cls_ph(ccls)) * (1 + cls_pw(ccls));
        }
    };

    Tile t0, t1, t2;
    load_tiles(t0);
    load_tiles(t1);                                      // nit >= 9
    load_tiles(t2);
    store_tiles(0, t0);
    lds_barrier();
    if constexpr (!PIPE) {
        for (int it = 0; it < nit; it += 3) {            // nit = 9 * nci: a multiple of 3
            tap_body(it, t0, t1);
            tap_body(it + 1, t1, t2);
            tap_body(it + 2, t2, t0);
        }
    } else {
        read_frag(fa, 0, 0);
        for (int it = 0; it < nit; it += 3) {
            tap_body0(it, t0, t1);
            tap_body0(it + 1, t1, t2);
            tap_body0(it + 2, t2, t0);
        }
    }
}

template <int BN, bool BWD>
int launch_conv3x3_s2(const void* src, const void* wp, void* dst, int M, int OH, int OW, int K, int NO, hipStream_t st) {
    const int MT = (M + S2_BM - 1) / S2_BM, NT = NO / BN;
    const size_t lds = (size_t)2 * (S2_BM + BN) * C3_LS * sizeof(bf16_t);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)conv3x3_s2_kernel<BN, BWD>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((conv3x3_s2_kernel<BN, BWD>), dim3((unsigned)(MT * NT)), dim3(256), lds, st,
                       (const bf16_t*)src, (const bf16_t*)wp, (bf16_t*)dst, M, OH, OW, K, NO, MT, NT);
    ADIL_CHECK_LAUNCH();
    return 0;
}

// what both entry points cover; M = rows of the stride-2 grid
bool conv3x3_s2_covers(int B, int H, int W, int C, int N, int* M) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0 || (H & 1) || (W & 1) || (C % 64) || (N % 64) || W > ADIL_CONV3X3_S2_MAX_W)
        return false;
    const long long m4 = (long long)B * H * W;           // rows of the full grid: every index is an int
    if (m4 > 0x7fffffffLL) return false;
    if (9LL * C * N > 0x7fffffffLL) return false;        // weight offsets are 32-bit element indices
    *M = (int)(m4 / 4);
    return true;
}

}  // namespace

extern "C" int adil_conv3x3_s2_fwd(const void* x, const void* wp, void* y, int B, int H, int W, int C, int N, void* stream) {
    ADIL_ENTER();
    int M = 0;
    if (!x || !wp || !y || !conv3x3_s2_covers(B, H, W, C, N, &M)) return ADIL_EINVAL;
    if (N % 128 == 0) return launch_conv3x3_s2<128, false>(x, wp, y, M, H / 2, W / 2, C, N, (hipStream_t)stream);
    return launch_conv3x3_s2<64, false>(x, wp, y, M, H / 2, W / 2, C, N, (hipStream_t)stream);
}

extern "C" int adil_conv3x3_s2_bwd(const void* g, const void* wp_bwd, void* gx, int B, int H, int W, int C, int N, void* stream) {
    ADIL_ENTER();
    int M = 0;
    if (!g || !wp_bwd || !gx || !conv3x3_s2_covers(B, H, W, C, N, &M)) return ADIL_EINVAL;
    if (C % 128 == 0) return launch_conv3x3_s2<128, true>(g, wp_bwd, gx, M, H / 2, W / 2, N, C, (hipStream_t)stream);
    return launch_conv3x3_s2<64, true>(g, wp_bwd, gx, M, H / 2, W / 2, N, C, (hipStream_t)stream);
}
