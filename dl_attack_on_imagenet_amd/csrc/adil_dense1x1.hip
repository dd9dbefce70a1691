// Pre-activated pointwise (1x1, stride 1) convolutions of the frozen DenseNet-121 — BatchNorm + ReLU IN FRONT of the
// convolution, on a concatenated input of K = 64 .. 1024 channels in steps of 32 — with the eval-BatchNorm and the ReLU
// behind it applied on the accumulators, forward and input gradient: adil_dense1x1_fwd / adil_dense1x1_bwd
// (include/adil_hip.h).  bf16 channels_last storage, bf16 MFMA with fp32 accumulation, one rounding to bf16 (RNE), no
// atomics, 64-bit element offsets.  The tile, its tails and the MFMA roles are those of adil_pw_tile.h; this file has what
// is d1_kernel's own.
//
// Both directions are the GEMM  OUT[M][O] = A'[M][R] . B[O][R]^T  of adil_pw_tile.h:
//   forward    A' = a = bf16(max(pre, 0)), pre = pw_preact(x, pscale[k], pshift[k]) formed on the way from registers to
//              LDS (two fp32 roundings, never one fma: the branch pre > 0 is the one the gradient recomputes);
//              R = K, B = w [N][K], O = N;  epilogue act(acc * scale[n] + shift[n]), act = max(., 0) or the identity
//   gradient   A' = gz = bf16(g * scale[n]) & [y > 0] formed the same way (the mask compares VALUES: -0.0 in y is a
//              zero); R = N, B = wt [K][N], O = K;  epilogue gx = [pre > 0] acc * pscale[k], pre recomputed from xin,
//              whose loads fly under the reduction loop
//   The 128 output channels of every dense layer are ONE tile: x crosses HBM once.
//   The per-reduction-channel tables (pscale | pshift, or scale) sit in LDS behind the tiles, zero-filled behind R; the
//   per-output-channel tables of this tile in a small static array.  A table entry past its extent is read at a clamped
//   index.  The tables are read element-wise (4-byte alignment is all they need).
//   Row pitches (the _ld entry points): x / g, y, xin and the output each have a pitch of their own, in elements, at or
//   above their width; row m of an operand starts at base + m * ld and the columns at or behind the width are never
//   touched (the clamped reads of the tails stay inside the width).  The weights and the tables are dense.  The plain
//   entry points pass ld = width.
//   ACC (gradient only): gx[m][k] = bf16_rne(f32(gx_old[m][k]) + v), v the fp32 value the plain gradient rounds: one fp32
//   add (never contracted with the product in front of it), one rounding.  The old value is fetched with xin, under the
//   reduction loop, by the lane that holds the accumulator; the wave that read a pixel row is the wave that writes it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adil_common.h"
#include "adil_hip.h"
#include "adil_mfma.h"
#include "adil_pw_tile.h"

namespace {

template <int CT, bool BWD, bool ACC>
__global__ __launch_bounds__(256) void d1_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ yin,
                                                 const bf16_t* __restrict__ bm, const float* __restrict__ rt0,
                                                 const float* __restrict__ rt1, const float* __restrict__ ot0,
                                                 const float* __restrict__ ot1, const bf16_t* __restrict__ xin,
                                                 bf16_t* __restrict__ out, int M, int R, int O, int act, int MT, int OT,
                                                 int tab_off, int lda, int ldyin, int ldxin, int ldo) {
    constexpr int BO = 32 * CT, ACH = PW_ACH, OS = BO + 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sa = reinterpret_cast<bf16_t*>(smem_raw);    // [128][PW_LS]
    bf16_t* sb = sa + PW_BM * PW_LS;                     // [BO][PW_LS]
    // per reduction channel, zeros behind R: forward pscale | pshift, gradient scale
    float* rtab = reinterpret_cast<float*>(smem_raw + tab_off);
    // per output channel of this tile: forward scale | shift, gradient pscale | pshift
    __shared__ float otab[2 * BO];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    int mt, ot;
    pw_tile_order(MT, OT, mt, ot);
    const int m0 = mt * PW_BM, o0 = ot * BO;
    const int nk = (R + PW_BK - 1) / PW_BK, RP = nk * PW_BK;
    for (int i = tid; i < RP; i += 256) {
        const bool ok = i < R;
        const int ic = ok ? i : 0;
        const float v0 = rt0[ic];
        rtab[i] = ok ? v0 : 0.0f;
        if (!BWD) {
            const float v1 = rt1[ic];
            rtab[RP + i] = ok ? v1 : 0.0f;
        }
    }
    if (tid < BO) {
        const int n = o0 + tid < O ? o0 + tid : O - 1;
        otab[tid] = ot0[n];
        otab[BO + tid] = ot1[n];
    }
    __syncthreads();

    const bool masked = BWD && act != 0;
    size_t arow[ACH], yrow[BWD ? ACH : 1];
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
        const int row = (tid + 256 * i) >> 3;
        const size_t mr = (size_t)((m0 + row < M) ? m0 + row : M - 1);
        arow[i] = mr * (size_t)lda;
        if (BWD) yrow[i] = mr * (size_t)ldyin;
    }
    u32x4 ar[ACH], yr[BWD ? ACH : 1], br[CT];
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const PwBTile<CT> bt{br, bm, sb, o0, O, R, tid};
    auto load_tiles = [&](int kc) {
        bool cok;
        const int colc = bt.column(kc, cok);
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            ar[i] = *reinterpret_cast<const u32x4*>(a + arow[i] + colc);
            if (masked) yr[i] = *reinterpret_cast<const u32x4*>(yin + yrow[i] + colc);
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
        const float* t0 = rtab + kc * PW_BK + ch * 8;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int row = (tid + 256 * i) >> 3;
            float v[8];
            unpack8(ar[i], v);
            u32x4 t;
            if (BWD) {
                float yv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= t0[e];
                t = pack8(v);
                if (masked) {
                    unpack8(yr[i], yv);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const unsigned lo = yv[2 * j] > 0.0f ? 0x0000ffffu : 0u;
                        const unsigned hi = yv[2 * j + 1] > 0.0f ? 0xffff0000u : 0u;
                        t[j] &= lo | hi;
                    }
                }
            } else {
                // a zero-filled chunk past R meets zero table entries: pre = 0, a = +0
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float pre = pw_preact(v[e], t0[e], t0[RP + e]);
                    v[e] = pre > 0.0f ? pre : 0.0f;      // <= 0 (and -0.0, and NaN) -> +0
                }
                t = pack8(v);
            }
            *reinterpret_cast<u32x4*>(sa + row * PW_LS + ch * 8) = t;
        }
        bt.store();
    };

    load_tiles(0);
    const int m = m0 + w * 32 + c;                       // this lane's pixel in the epilogue
    // the gradient's xin does not depend on the GEMM: its loads fly under the reduction loop
    u32x2 xr[BWD ? CT : 1][4], gr[ACC ? CT : 1][4];
    if (BWD) {
        const bf16_t* xp = xin + (size_t)(m < M ? m : M - 1) * (size_t)ldxin;
        const bf16_t* gp = out + (size_t)(m < M ? m : M - 1) * (size_t)ldo;        // the old gradient (ACC)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = o0 + 32 * ct + 8 * q + 4 * h;          // O % 8 == 0: the four channels are in or out together
                xr[ct][q] = *reinterpret_cast<const u32x2*>(xp + (n < O ? n : 0));
                if (ACC) gr[ct][q] = *reinterpret_cast<const u32x2*>(gp + (n < O ? n : 0));
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
            if (BWD) {
                const f32x2 x0 = bf2_to_f32x2(xr[ct][q][0]), x1 = bf2_to_f32x2(xr[ct][q][1]);
                const float xv[4] = {x0[0], x0[1], x1[0], x1[1]};
                if (ACC) {
                    const f32x2 g0 = bf2_to_f32x2(gr[ct][q][0]), g1 = bf2_to_f32x2(gr[ct][q][1]);
                    const float gv[4] = {g0[0], g0[1], g1[0], g1[1]};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float ps = otab[co + e];
                        const float pre = pw_preact(xv[e], ps, otab[BO + co + e]);
                        // old + v, v = +0 off the forward's branch (an old -0.0 there becomes +0)
                        v[e] = pre > 0.0f ? pw_mul_add(v[e], ps, gv[e]) : gv[e] + 0.0f;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float ps = otab[co + e];
                        const float pre = pw_preact(xv[e], ps, otab[BO + co + e]);
                        v[e] = pre > 0.0f ? v[e] * ps : 0.0f;        // the forward's branch; elsewhere +0
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = v[e] * otab[co + e] + otab[BO + co + e];
                if (act) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.0f ? v[e] : 0.0f;      // <= 0 (and -0.0) -> +0
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
        if (mm < M && n < O) *reinterpret_cast<u32x4*>(out + (size_t)mm * (size_t)ldo + n) = t;
    }
}

// one call: the operands of the GEMM OUT[M][O] = A'[M][R] . B[O][R]^T with their row pitches (elements)
struct D1Call {
    const bf16_t *a, *yin, *bm, *xin;
    const float *rt0, *rt1, *ot0, *ot1;
    bf16_t* out;
    int M, R, O, act, lda, ldyin, ldxin, ldo;
};

template <bool BWD, bool ACC>
void d1_dispatch(const D1Call& c, hipStream_t s) {
    pw_dispatch(c.O, [&](auto ct, int OT) {
        constexpr int CT = decltype(ct)::value;
        constexpr size_t tab_off = pw_tile_bytes<CT>();
        const int MT = pw_pixel_tiles(c.M), RP = (c.R + PW_BK - 1) / PW_BK * PW_BK;
        const size_t tabs = (size_t)(BWD ? 1 : 2) * RP * sizeof(float);
        // widest case (CT = 5, forward, R = 2048): 43008 B of transposed output + 16384 B of tables + 1280 B of static otab
        // = 60672 B of the 64 KiB a workgroup may have
        static_assert(tab_off % 16 == 0 && tab_off + 2 * PW_MAXC * sizeof(float) + 2 * 32 * CT * sizeof(float) <= 65536,
                      "tiles + reduction tables + otab must fit the 64 KiB of LDS a workgroup may have");
        hipLaunchKernelGGL((d1_kernel<CT, BWD, ACC>), dim3((unsigned)MT * (unsigned)OT), dim3(256), tab_off + tabs, s, c.a,
                           c.yin, c.bm, c.rt0, c.rt1, c.ot0, c.ot1, c.xin, c.out, c.M, c.R, c.O, c.act, MT, OT, (int)tab_off,
                           c.lda, c.ldyin, c.ldxin, c.ldo);
    });
}

}  // namespace

extern "C" int adil_dense1x1_fwd_ld(const void* x, int ldx, const float* pscale, const float* pshift, const void* w,
                                    const float* scale, const float* shift, void* y, int ldy, int M, int K, int N, int act,
                                    void* stream) {
    if (x == nullptr || pscale == nullptr || pshift == nullptr || w == nullptr || scale == nullptr || shift == nullptr ||
        y == nullptr || !pw_dims_ok(M, K, N, act) || !pw_ld_ok(ldx, K) || !pw_ld_ok(ldy, N))
        return ADIL_EINVAL;
    if (!aligned(x, 16) || !aligned(w, 16) || !aligned(y, 16) || !aligned(pscale, 4) || !aligned(pshift, 4) ||
        !aligned(scale, 4) || !aligned(shift, 4))
        return ADIL_EINVAL;
    ADIL_ENTER();
    const D1Call c = {(const bf16_t*)x, nullptr, (const bf16_t*)w, nullptr, pscale, pshift, scale, shift, (bf16_t*)y,
                      M, K, N, act, ldx, 0, 0, ldy};
    d1_dispatch<false, false>(c, (hipStream_t)stream);
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_dense1x1_fwd(const void* x, const float* pscale, const float* pshift, const void* w, const float* scale,
                                 const float* shift, void* y, int M, int K, int N, int act, void* stream) {
    return adil_dense1x1_fwd_ld(x, K, pscale, pshift, w, scale, shift, y, N, M, K, N, act, stream);
}

extern "C" int adil_dense1x1_bwd_ld(const void* g, int ldg, const void* y, int ldy, const float* scale, const void* wt,
                                    const void* xin, int ldxin, const float* pscale, const float* pshift, void* gx, int ldgx,
                                    int accumulate, int M, int K, int N, int act, void* stream) {
    if (g == nullptr || scale == nullptr || wt == nullptr || xin == nullptr || pscale == nullptr || pshift == nullptr ||
        gx == nullptr || !pw_dims_ok(M, K, N, act) || !pw_ld_ok(ldg, N) || !pw_ld_ok(ldy, N) || !pw_ld_ok(ldxin, K) ||
        !pw_ld_ok(ldgx, K) || (accumulate != 0 && accumulate != 1))
        return ADIL_EINVAL;
    if (act != 0 && y == nullptr) return ADIL_EINVAL;
    if (!aligned(g, 16) || !aligned(wt, 16) || !aligned(xin, 16) || !aligned(gx, 16) || (act != 0 && !aligned(y, 16)) ||
        !aligned(scale, 4) || !aligned(pscale, 4) || !aligned(pshift, 4))
        return ADIL_EINVAL;
    ADIL_ENTER();
    const D1Call c = {(const bf16_t*)g, act ? (const bf16_t*)y : nullptr, (const bf16_t*)wt, (const bf16_t*)xin, scale, nullptr,
                      pscale, pshift, (bf16_t*)gx, M, N, K, act, ldg, ldy, ldxin, ldgx};
    if (accumulate)
        d1_dispatch<true, true>(c, (hipStream_t)stream);
    else
        d1_dispatch<true, false>(c, (hipStream_t)stream);
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_dense1x1_bwd(const void* g, const void* y, const float* scale, const void* wt, const void* xin,
                                 const float* pscale, const float* pshift, void* gx, int M, int K, int N, int act,
                                 void* stream) {
    return adil_dense1x1_bwd_ld(g, N, y, N, scale, wt, xin, K, pscale, pshift, gx, K, 0, M, K, N, act, stream);
}
