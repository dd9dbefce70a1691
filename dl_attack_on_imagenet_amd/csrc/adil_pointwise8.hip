// Pointwise (1x1, stride 1) convolutions of the frozen MobileNetV2 — channel counts that are multiples of 8, not of 64
// (16 / 24 / 32 / 96 / 144 / 160 / 192 / 320 / 384 / 576 / 960 / 1280) — with the eval-BatchNorm, the optional residual
// add and the ReLU6 clamp applied on the accumulators, forward and input gradient: adil_pw8_fwd / adil_pw8_bwd
// (include/adil_hip.h).  bf16 channels_last storage, bf16 MFMA with fp32 accumulation, one rounding to bf16 (RNE), no
// atomics, 64-bit element offsets.
//
// Both directions are the row-major GEMM  OUT[M][O] = A'[M][R] . B[O][R]^T  (M = pixels):
//   forward    A' = x,  R = K, B = w [N][K],  O = N;  epilogue act(acc * scale[n] + shift[n] (+ res))
//   gradient   A' = gz, R = N, B = wt [K][N], O = K;  gz = bf16(g * scale[n]) & [0 < y < 6] formed on the way from
//              registers to LDS (one fp32 product, one rounding; the mask compares VALUES, so -0.0 in y is a zero)
// and both are HBM streams: what matters is that an activation crosses HBM once, in 16-byte accesses.
//   Workgroup = 4 waves = 128 pixels x BO output channels, BO = 32 CT with CT = 1 .. 5 picked on the host so that the
//   fewest channel tiles cover O (one tile up to O = 160: every projection and every narrow layer reads its input once).
//   The reduction runs in chunks of 64 through LDS, the next chunk waiting in registers, in MFMA steps of 16; only the
//   steps the chunk holds are issued (R = 16 is one step).
//   MFMA roles as in adil_convs.hip: A operand = B rows (channels -> accumulator registers), B operand = pixels ->
//   lanes; a lane owns 4 consecutive channels of one pixel per register quad; the finished tile goes through a per-wave
//   LDS transpose to 16-byte stores.
//   Tails are clipped and zero-filled, never read from a neighbour: a 16-byte chunk past R (R % 8 == 0: a chunk is
//   wholly inside or wholly outside) and a B row past O are read at a clamped in-range address and replaced by zeros on
//   BOTH operands (0 x NaN would be NaN); a pixel row past M reads row M - 1 and is not stored.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adil_common.h"
#include "adil_hip.h"
#include "adil_mfma.h"

namespace {

#define P8_BM 128
#define P8_BK 64
#define P8_LS (P8_BK + 8)              // LDS row stride (elements): 144 B = 9 x 16 B
#define P8_MAXC 2048

template <int CT, bool BWD, bool RES>
__global__ __launch_bounds__(256) void pw8_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ yin,
                                                  const bf16_t* __restrict__ bm, const float* __restrict__ scale,
                                                  const float* __restrict__ shift, const bf16_t* __restrict__ res,
                                                  bf16_t* __restrict__ out, int M, int R, int O, int act, int MT, int OT) {
    constexpr int BO = 32 * CT;
    constexpr int ACH = P8_BM * P8_BK / 8 / 256;         // 16-byte chunks of the A tile per thread (4)
    constexpr int OS = BO + 8;                           // transposed-output pixel stride (elements)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sa = reinterpret_cast<bf16_t*>(smem_raw);    // [128][P8_LS]
    bf16_t* sb = sa + P8_BM * P8_LS;                     // [BO][P8_LS]
    // forward: this tile's scale | shift; gradient: the scale of every reduction channel, zeros behind R
    __shared__ __attribute__((aligned(16))) float stab[BWD ? P8_MAXC : 2 * BO];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    // workgroups are dealt round-robin to the 8 XCDs: the OT channel tiles of one pixel tile go to ONE XCD, so the
    // repeated reads of an A tile meet in that XCD's L2.  Pixel tiles behind the last multiple of 8 keep the plain order.
    int mt, ot;
    {
        const int id = blockIdx.x, full = (MT >> 3) * 8 * OT;
        if (id < full) {
            const int xcd = id & 7, j = id >> 3;
            ot = j % OT;
            mt = (j / OT) * 8 + xcd;
        } else {
            const int r = id - full;
            ot = r % OT;
            mt = (MT >> 3) * 8 + r / OT;
        }
    }
    const int m0 = mt * P8_BM, o0 = ot * BO;
    const int nk = (R + P8_BK - 1) / P8_BK;
    if (BWD) {
#pragma unroll
        for (int j = 0; j < P8_MAXC / 4 / 256; ++j) {
            const int i4 = tid + 256 * j;
            float4 v = *reinterpret_cast<const float4*>(scale + (4 * i4 < R ? 4 * i4 : 0));
            if (4 * i4 >= R) v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            *reinterpret_cast<float4*>(stab + 4 * i4) = v;
        }
    } else if (tid < BO) {
        const int n = o0 + tid < O ? o0 + tid : O - 1;
        stab[tid] = scale[n];
        stab[BO + tid] = shift[n];
    }
    __syncthreads();

    size_t arow[ACH];
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
        const int row = (tid + 256 * i) >> 3;
        arow[i] = (size_t)((m0 + row < M) ? m0 + row : M - 1) * (size_t)R;
    }
    const bool masked = BWD && act != 0;
    u32x4 ar[ACH], yr[BWD ? ACH : 1], br[CT];
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    auto load_tiles = [&](int kc) {
        const int col = kc * P8_BK + (tid & 7) * 8;      // the same 16-byte column for every chunk of this thread
        const bool cok = col < R;
        const int colc = cok ? col : 0;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            ar[i] = *reinterpret_cast<const u32x4*>(a + arow[i] + colc);
            if (masked) yr[i] = *reinterpret_cast<const u32x4*>(yin + arow[i] + colc);
            if (!cok) ar[i] = zero4;
        }
#pragma unroll
        for (int i = 0; i < CT; ++i) {
            const int n = o0 + ((tid + 256 * i) >> 3);
            const bool ok = cok && n < O;
            br[i] = *reinterpret_cast<const u32x4*>(bm + (ok ? (size_t)n * (size_t)R + colc : (size_t)0));
            if (!ok) br[i] = zero4;
        }
    };
    auto store_tiles = [&](int kc) {
        const int ch = tid & 7;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int row = (tid + 256 * i) >> 3;
            u32x4 t = ar[i];
            if (BWD) {
                float gv[8], yv[8];
                unpack8(ar[i], gv);
                const float* sc = stab + kc * P8_BK + ch * 8;
#pragma unroll
                for (int e = 0; e < 8; ++e) gv[e] *= sc[e];
                t = pack8(gv);
                if (masked) {
                    unpack8(yr[i], yv);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const unsigned lo = (yv[2 * j] > 0.0f && yv[2 * j] < 6.0f) ? 0x0000ffffu : 0u;
                        const unsigned hi = (yv[2 * j + 1] > 0.0f && yv[2 * j + 1] < 6.0f) ? 0xffff0000u : 0u;
                        t[j] &= lo | hi;
                    }
                }
            }
            *reinterpret_cast<u32x4*>(sa + row * P8_LS + ch * 8) = t;
        }
#pragma unroll
        for (int i = 0; i < CT; ++i) {
            const int row = (tid + 256 * i) >> 3;
            *reinterpret_cast<u32x4*>(sb + row * P8_LS + ch * 8) = br[i];
        }
    };

    load_tiles(0);
    const int m = m0 + w * 32 + c;                       // this lane's pixel in the epilogue
    // the residual does not depend on the GEMM: its loads fly under the K loop
    u32x2 rr[RES ? CT : 1][4];
    if (RES) {
        const bf16_t* rp = res + (size_t)(m < M ? m : M - 1) * (size_t)O;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = o0 + 32 * ct + 8 * q + 4 * h;          // O % 8 == 0: the four channels are in or out together
                rr[ct][q] = *reinterpret_cast<const u32x2*>(rp + (n < O ? n : 0));
            }
    }
    f32x16 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.0f;
    for (int it = 0; it < nk; ++it) {
        store_tiles(it);
        if (it + 1 < nk) load_tiles(it + 1);
        lds_barrier();
        const bf16_t* bx = sa + (w * 32 + c) * P8_LS + 8 * h;
        const bf16_t* bw = sb + c * P8_LS + 8 * h;
        const int left = R - it * P8_BK;
        const int steps = left >= P8_BK ? P8_BK / 16 : (left + 15) / 16;
        for (int ks = 0; ks < steps; ++ks) {
            const bf16x8 b = lds8(bx + 16 * ks);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) mma16(acc[ct], lds8(bw + ct * 32 * P8_LS + 16 * ks), b);
        }
        lds_barrier();
    }
    // epilogue on the accumulators: lane = pixel m, register quad q of tile ct = channels o0 + 32ct + 8q + 4h .. +3
    bf16_t* so = reinterpret_cast<bf16_t*>(smem_raw) + w * 32 * OS;     // the tile buffers are idle now
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int co = 32 * ct + 8 * q + 4 * h;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[ct][4 * q + e];
            if (!BWD) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = v[e] * stab[co + e] + stab[BO + co + e];
                if (RES) {
                    const f32x2 r0 = bf2_to_f32x2(rr[ct][q][0]), r1 = bf2_to_f32x2(rr[ct][q][1]);
                    v[0] += r0[0]; v[1] += r0[1]; v[2] += r1[0]; v[3] += r1[1];
                }
                if (act) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fminf(v[e] > 0.0f ? v[e] : 0.0f, 6.0f);   // <= 0 (and -0.0) -> +0
                }
            }
            u32x2 t;
            t[0] = pack2_bf16(v[0], v[1]);
            t[1] = pack2_bf16(v[2], v[3]);
            *reinterpret_cast<u32x2*>(so + c * OS + co) = t;
        }
    }
    constexpr int CPP = BO / 8;                          // 16-byte chunks per pixel
#pragma unroll
    for (int i = 0; i < 32 * CPP / 64; ++i) {
        const int id = lane + 64 * i, px = id / CPP, ch = id - px * CPP;
        const u32x4 t = *reinterpret_cast<const u32x4*>(so + px * OS + ch * 8);
        const int mm = m0 + w * 32 + px, n = o0 + ch * 8;
        if (mm < M && n < O) *reinterpret_cast<u32x4*>(out + (size_t)mm * (size_t)O + n) = t;
    }
}

inline bool p8_dims_ok(int M, int K, int N, int act) {
    return M >= 1 && K >= 8 && N >= 8 && K <= P8_MAXC && N <= P8_MAXC && (K % 8) == 0 && (N % 8) == 0 && (act == 0 || act == 1);
}

template <int CT, bool BWD, bool RES>
void p8_launch(const bf16_t* a, const bf16_t* yin, const bf16_t* bm, const float* scale, const float* shift,
               const bf16_t* res, bf16_t* out, int M, int R, int O, int act, int OT, hipStream_t s) {
    constexpr int BO = 32 * CT;
    constexpr size_t tiles = (size_t)(P8_BM + BO) * P8_LS * sizeof(bf16_t), trans = (size_t)4 * 32 * (BO + 8) * sizeof(bf16_t);
    const int MT = (M + P8_BM - 1) / P8_BM;
    hipLaunchKernelGGL((pw8_kernel<CT, BWD, RES>), dim3((unsigned)MT * (unsigned)OT), dim3(256), tiles > trans ? tiles : trans, s,
                       a, yin, bm, scale, shift, res, out, M, R, O, act, MT, OT);
}

// fewest channel tiles of at most 160 channels that cover O, and the narrowest tile that does it
template <bool BWD, bool RES>
void p8_dispatch(const bf16_t* a, const bf16_t* yin, const bf16_t* bm, const float* scale, const float* shift,
                 const bf16_t* res, bf16_t* out, int M, int R, int O, int act, hipStream_t s) {
    const int OT = (O + 159) / 160, per = (O + OT - 1) / OT, ct = (per + 31) / 32;
    switch (ct) {
        case 1: p8_launch<1, BWD, RES>(a, yin, bm, scale, shift, res, out, M, R, O, act, OT, s); break;
        case 2: p8_launch<2, BWD, RES>(a, yin, bm, scale, shift, res, out, M, R, O, act, OT, s); break;
        case 3: p8_launch<3, BWD, RES>(a, yin, bm, scale, shift, res, out, M, R, O, act, OT, s); break;
        case 4: p8_launch<4, BWD, RES>(a, yin, bm, scale, shift, res, out, M, R, O, act, OT, s); break;
        default: p8_launch<5, BWD, RES>(a, yin, bm, scale, shift, res, out, M, R, O, act, OT, s); break;
    }
}

}  // namespace

extern "C" int adil_pw8_fwd(const void* x, const void* w, const float* scale, const float* shift, const void* res, void* y,
                            int M, int K, int N, int act, void* stream) {
    if (x == nullptr || w == nullptr || scale == nullptr || shift == nullptr || y == nullptr || !p8_dims_ok(M, K, N, act))
        return ADIL_EINVAL;
    if (res != nullptr && act != 0) return ADIL_EINVAL;
    if (!aligned(x, 16) || !aligned(w, 16) || !aligned(scale, 16) || !aligned(shift, 16) || !aligned(res, 16) || !aligned(y, 16))
        return ADIL_EINVAL;
    ADIL_ENTER();
    hipStream_t s = (hipStream_t)stream;
    if (res != nullptr)
        p8_dispatch<false, true>((const bf16_t*)x, nullptr, (const bf16_t*)w, scale, shift, (const bf16_t*)res, (bf16_t*)y, M, K, N,
                                 act, s);
    else
        p8_dispatch<false, false>((const bf16_t*)x, nullptr, (const bf16_t*)w, scale, shift, nullptr, (bf16_t*)y, M, K, N, act, s);
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_pw8_bwd(const void* g, const void* y, const float* scale, const void* wt, void* gx, int M, int K, int N,
                            int act, void* stream) {
    if (g == nullptr || scale == nullptr || wt == nullptr || gx == nullptr || !p8_dims_ok(M, K, N, act)) return ADIL_EINVAL;
    if (act != 0 && y == nullptr) return ADIL_EINVAL;
    if (!aligned(g, 16) || !aligned(scale, 16) || !aligned(wt, 16) || !aligned(gx, 16) || (act != 0 && !aligned(y, 16)))
        return ADIL_EINVAL;
    ADIL_ENTER();
    p8_dispatch<true, false>((const bf16_t*)g, act ? (const bf16_t*)y : nullptr, (const bf16_t*)wt, scale, nullptr, nullptr,
                             (bf16_t*)gx, M, N, K, act, (hipStream_t)stream);
    ADIL_CHECK_LAUNCH();
    return 0;
}
