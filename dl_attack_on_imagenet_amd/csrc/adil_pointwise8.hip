// Pointwise (1x1, stride 1) convolutions of the frozen MobileNetV2 — channel counts that are multiples of 8, not of 64
// (16 / 24 / 32 / 96 / 144 / 160 / 192 / 320 / 384 / 576 / 960 / 1280) — with the eval-BatchNorm, the optional residual
// add and the ReLU6 clamp applied on the accumulators, forward and input gradient: adil_pw8_fwd / adil_pw8_bwd
// (include/adil_hip.h).  bf16 channels_last storage, bf16 MFMA with fp32 accumulation, one rounding to bf16 (RNE), no
// atomics, 64-bit element offsets.  The tile, its tails and the MFMA roles are those of adil_pw_tile.h; this file has what
// is pw8_kernel's own.
//
// Both directions are the GEMM  OUT[M][O] = A'[M][R] . B[O][R]^T  of adil_pw_tile.h:
//   forward    A' = x,  R = K, B = w [N][K],  O = N;  epilogue act(acc * scale[n] + shift[n] (+ res))
//   gradient   A' = gz, R = N, B = wt [K][N], O = K;  gz = bf16(g * scale[n]) & [0 < y < 6] formed on the way from
//              registers to LDS (one fp32 product, one rounding; the mask compares VALUES, so -0.0 in y is a zero)
//   The operands are dense (no row pitches).  The tables sit in a static array, filled in 16-byte loads in the gradient:
//   the ABI asks for 16-byte aligned scale and shift.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adil_common.h"
#include "adil_hip.h"
#include "adil_mfma.h"
#include "adil_pw_tile.h"

namespace {

template <int CT, bool BWD, bool RES>
__global__ __launch_bounds__(256) void pw8_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ yin,
                                                  const bf16_t* __restrict__ bm, const float* __restrict__ scale,
                                                  const float* __restrict__ shift, const bf16_t* __restrict__ res,
                                                  bf16_t* __restrict__ out, int M, int R, int O, int act, int MT, int OT) {
    constexpr int BO = 32 * CT, ACH = PW_ACH, OS = BO + 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sa = reinterpret_cast<bf16_t*>(smem_raw);    // [128][PW_LS]
    bf16_t* sb = sa + PW_BM * PW_LS;                     // [BO][PW_LS]
    // forward: this tile's scale | shift; gradient: the scale of every reduction channel, zeros behind R
    __shared__ __attribute__((aligned(16))) float stab[BWD ? PW_MAXC : 2 * BO];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    int mt, ot;
    pw_tile_order(MT, OT, mt, ot);
    const int m0 = mt * PW_BM, o0 = ot * BO;
    const int nk = (R + PW_BK - 1) / PW_BK;
    if (BWD) {
#pragma unroll
        for (int j = 0; j < PW_MAXC / 4 / 256; ++j) {
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
    const PwBTile<CT> bt{br, bm, sb, o0, O, R, tid};
    auto load_tiles = [&](int kc) {
        bool cok;
        const int colc = bt.column(kc, cok);
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            ar[i] = *reinterpret_cast<const u32x4*>(a + arow[i] + colc);
            if (masked) yr[i] = *reinterpret_cast<const u32x4*>(yin + arow[i] + colc);
            if (!cok) ar[i] = zero4;
        }
        // the B tile, as PwBTile::load has it (written out here: see adil_pw_tile.h)
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
                const float* sc = stab + kc * PW_BK + ch * 8;
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
            *reinterpret_cast<u32x4*>(sa + row * PW_LS + ch * 8) = t;
        }
        bt.store();
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
    pw_clear(acc);
    for (int it = 0; it < nk; ++it) {
        store_tiles(it);
        if (it + 1 < nk) load_tiles(it + 1);
        lds_barrier();
        // pw_mma_chunk, written out here (see adil_pw_tile.h)
        const bf16_t* bx = sa + (w * 32 + c) * PW_LS + 8 * h;
        const bf16_t* bw = sb + c * PW_LS + 8 * h;
        const int left = R - it * PW_BK;
        const int steps = left >= PW_BK ? PW_BK / 16 : (left + 15) / 16;
        for (int ks = 0; ks < steps; ++ks) {
            const bf16x8 b = lds8(bx + 16 * ks);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) mma16(acc[ct], lds8(bw + ct * 32 * PW_LS + 16 * ks), b);
        }
        lds_barrier();
    }
    bf16_t* so = reinterpret_cast<bf16_t*>(smem_raw) + w * 32 * OS;     // the tile buffers are idle now
    // pw_stage, written out here (see adil_pw_tile.h): lane = pixel m, register quad q of tile ct = channels
    // o0 + 32ct + 8q + 4h .. +3
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
    // pw_write_out, written out here (see adil_pw_tile.h)
    constexpr int CPP = BO / 8;                          // 16-byte chunks per pixel
#pragma unroll
    for (int i = 0; i < 32 * CPP / 64; ++i) {
        const int id = lane + 64 * i, px = id / CPP, ch = id - px * CPP;
        const u32x4 t = *reinterpret_cast<const u32x4*>(so + px * OS + ch * 8);
        const int mm = m0 + w * 32 + px, n = o0 + ch * 8;
        if (mm < M && n < O) *reinterpret_cast<u32x4*>(out + (size_t)mm * (size_t)O + n) = t;
    }
}

template <bool BWD, bool RES>
void p8_dispatch(const bf16_t* a, const bf16_t* yin, const bf16_t* bm, const float* scale, const float* shift,
                 const bf16_t* res, bf16_t* out, int M, int R, int O, int act, hipStream_t s) {
    pw_dispatch(O, [&](auto ct, int OT) {
        constexpr int CT = decltype(ct)::value;
        const int MT = pw_pixel_tiles(M);
        hipLaunchKernelGGL((pw8_kernel<CT, BWD, RES>), dim3((unsigned)MT * (unsigned)OT), dim3(256), pw_tile_bytes<CT>(), s, a, yin,
                           bm, scale, shift, res, out, M, R, O, act, MT, OT);
    });
}

}  // namespace

extern "C" int adil_pw8_fwd(const void* x, const void* w, const float* scale, const float* shift, const void* res, void* y,
                            int M, int K, int N, int act, void* stream) {
    if (x == nullptr || w == nullptr || scale == nullptr || shift == nullptr || y == nullptr || !pw_dims_ok(M, K, N, act))
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
    if (g == nullptr || scale == nullptr || wt == nullptr || gx == nullptr || !pw_dims_ok(M, K, N, act)) return ADIL_EINVAL;
    if (act != 0 && y == nullptr) return ADIL_EINVAL;
    if (!aligned(g, 16) || !aligned(scale, 16) || !aligned(wt, 16) || !aligned(gx, 16) || (act != 0 && !aligned(y, 16)))
        return ADIL_EINVAL;
    ADIL_ENTER();
    p8_dispatch<true, false>((const bf16_t*)g, act ? (const bf16_t*)y : nullptr, (const bf16_t*)wt, scale, nullptr, nullptr,
                             (bf16_t*)gx, M, N, K, act, (hipStream_t)stream);
    ADIL_CHECK_LAUNCH();
    return 0;
}
