// Pre-activated pointwise (1x1, stride 1) convolutions of the frozen DenseNet-121 — BatchNorm + ReLU IN FRONT of the
// convolution, on a concatenated input of K = 64 .. 1024 channels in steps of 32 — with the eval-BatchNorm and the ReLU
// behind it applied on the accumulators, forward and input gradient: adil_dense1x1_fwd / adil_dense1x1_bwd
// (include/adil_hip.h).  bf16 channels_last storage, bf16 MFMA with fp32 accumulation, one rounding to bf16 (RNE), no
// atomics, 64-bit element offsets.  A sibling of adil_pointwise8.hip (same tiling, same MFMA roles, same tails), which
// stays as it is: the two differ in what happens on the way from registers to LDS and in the epilogue.
//
// Both directions are the row-major GEMM  OUT[M][O] = A'[M][R] . B[O][R]^T  (M = pixels):
//   forward    A' = a = bf16(max(pre, 0)), pre = fadd(fmul(x, pscale[k]), pshift[k]) formed on the way from registers to
//              LDS (two fp32 roundings, never one fma: the branch pre > 0 is the one the gradient recomputes);
//              R = K, B = w [N][K], O = N;  epilogue act(acc * scale[n] + shift[n]), act = max(., 0) or the identity
//   gradient   A' = gz = bf16(g * scale[n]) & [y > 0] formed the same way (the mask compares VALUES: -0.0 in y is a
//              zero); R = N, B = wt [K][N], O = K;  epilogue gx = [pre > 0] acc * pscale[k], pre recomputed from xin,
//              whose loads fly under the reduction loop
//   Workgroup = 4 waves = 128 pixels x BO output channels, BO = 32 CT with CT = 1 .. 5 picked on the host so that the
//   fewest channel tiles cover O (the 128 output channels of every dense layer are ONE tile: x crosses HBM once).
//   The reduction runs in chunks of 64 through LDS, the next chunk waiting in registers, in MFMA steps of 16; only the
//   steps the chunk holds are issued.  The per-reduction-channel tables (pscale | pshift, or scale) sit in LDS behind
//   the tiles, zero-filled behind R; the per-output-channel tables of this tile in a small static array.
//   Tails are clipped and zero-filled, never read from a neighbour: a 16-byte chunk past R (R % 8 == 0) and a B row past
//   O are read at a clamped in-range address and replaced by zeros on BOTH operands; a pixel row past M reads row M - 1
//   and is not stored; a table entry past its extent is read at a clamped index.  The tables are read element-wise
//   (4-byte alignment is all they need).
//   Row pitches (the _ld entry points): x / g, y, xin and the output each have a pitch of their own, in elements, at or
//   above their width; row m of an operand starts at base + m * ld and the columns at or behind the width are never
//   touched (the clamped reads above stay inside the width).  The weights and the tables are dense.  The plain entry
//   points pass ld = width.
//   ACC (gradient only): gx[m][k] = bf16_rne(f32(gx_old[m][k]) + v), v the fp32 value the plain gradient rounds: one fp32
//   add (never contracted with the product in front of it), one rounding.  The old value is fetched with xin, under the
//   reduction loop, by the lane that holds the accumulator; the wave that read a pixel row is the wave that writes it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adil_common.h"
#include "adil_hip.h"
#include "adil_mfma.h"

namespace {

#define D1_BM 128
#define D1_BK 64
#define D1_LS (D1_BK + 8)              // LDS row stride (elements): 144 B = 9 x 16 B
#define D1_MAXC 2048

// the pre-activation of one input element: the product and the sum are each rounded to fp32 (no contraction), so an
// fp32 restatement reproduces the value AND the branch pre > 0, in the forward and in the gradient alike.  The two
// operations are written out under the pragma: __fmul_rn / __fadd_rn are plain `*` and `+` in a header, outside the
// pragma's reach, and contract to one fma after inlining
__device__ __forceinline__ float d1_pre(float x, float ps, float pb) {
#pragma clang fp contract(off)
    const float p = x * ps;
    return p + pb;
}

// the accumulate form's value: the product is rounded to fp32 BEFORE the old gradient is added (no fma)
__device__ __forceinline__ float d1_mul_add(float t, float ps, float old) {
#pragma clang fp contract(off)
    const float v = t * ps;
    return old + v;
}

template <int CT, bool BWD, bool ACC>
__global__ __launch_bounds__(256) void d1_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ yin,
                                                 const bf16_t* __restrict__ bm, const float* __restrict__ rt0,
                                                 const float* __restrict__ rt1, const float* __restrict__ ot0,
                                                 const float* __restrict__ ot1, const bf16_t* __restrict__ xin,
                                                 bf16_t* __restrict__ out, int M, int R, int O, int act, int MT, int OT,
                                                 int tab_off, int lda, int ldyin, int ldxin, int ldo) {
    constexpr int BO = 32 * CT;
    constexpr int ACH = D1_BM * D1_BK / 8 / 256;         // 16-byte chunks of the A tile per thread (4)
    constexpr int OS = BO + 8;                           // transposed-output pixel stride (elements)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16_t* sa = reinterpret_cast<bf16_t*>(smem_raw);    // [128][D1_LS]
    bf16_t* sb = sa + D1_BM * D1_LS;                     // [BO][D1_LS]
    // per reduction channel, zeros behind R: forward pscale | pshift, gradient scale
    float* rtab = reinterpret_cast<float*>(smem_raw + tab_off);
    // per output channel of this tile: forward scale | shift, gradient pscale | pshift
    __shared__ float otab[2 * BO];
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
    const int m0 = mt * D1_BM, o0 = ot * BO;
    const int nk = (R + D1_BK - 1) / D1_BK, RP = nk * D1_BK;
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
    auto load_tiles = [&](int kc) {
        const int col = kc * D1_BK + (tid & 7) * 8;      // the same 16-byte column for every chunk of this thread
        const bool cok = col < R;
        const int colc = cok ? col : 0;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            ar[i] = *reinterpret_cast<const u32x4*>(a + arow[i] + colc);
            if (masked) yr[i] = *reinterpret_cast<const u32x4*>(yin + yrow[i] + colc);
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
        const float* t0 = rtab + kc * D1_BK + ch * 8;
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
                    const float pre = d1_pre(v[e], t0[e], t0[RP + e]);
                    v[e] = pre > 0.0f ? pre : 0.0f;      // <= 0 (and -0.0, and NaN) -> +0
                }
                t = pack8(v);
            }
            *reinterpret_cast<u32x4*>(sa + row * D1_LS + ch * 8) = t;
        }
#pragma unroll
        for (int i = 0; i < CT; ++i) {
            const int row = (tid + 256 * i) >> 3;
            *reinterpret_cast<u32x4*>(sb + row * D1_LS + ch * 8) = br[i];
        }
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
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.0f;
    for (int it = 0; it < nk; ++it) {
        store_tiles(it);
        if (it + 1 < nk) load_tiles(it + 1);
        lds_barrier();
        const bf16_t* bx = sa + (w * 32 + c) * D1_LS + 8 * h;
        const bf16_t* bw = sb + c * D1_LS + 8 * h;
        const int left = R - it * D1_BK;
        const int steps = left >= D1_BK ? D1_BK / 16 : (left + 15) / 16;
        for (int ks = 0; ks < steps; ++ks) {
            const bf16x8 b = lds8(bx + 16 * ks);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) mma16(acc[ct], lds8(bw + ct * 32 * D1_LS + 16 * ks), b);
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
            if (BWD) {
                const f32x2 x0 = bf2_to_f32x2(xr[ct][q][0]), x1 = bf2_to_f32x2(xr[ct][q][1]);
                const float xv[4] = {x0[0], x0[1], x1[0], x1[1]};
                if (ACC) {
                    const f32x2 g0 = bf2_to_f32x2(gr[ct][q][0]), g1 = bf2_to_f32x2(gr[ct][q][1]);
                    const float gv[4] = {g0[0], g0[1], g1[0], g1[1]};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float ps = otab[co + e];
                        const float pre = d1_pre(xv[e], ps, otab[BO + co + e]);
                        // old + v, v = +0 off the forward's branch (an old -0.0 there becomes +0)
                        v[e] = pre > 0.0f ? d1_mul_add(v[e], ps, gv[e]) : gv[e] + 0.0f;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float ps = otab[co + e];
                        const float pre = d1_pre(xv[e], ps, otab[BO + co + e]);
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
    constexpr int CPP = BO / 8;                          // 16-byte chunks per pixel
#pragma unroll
    for (int i = 0; i < 32 * CPP / 64; ++i) {
        const int id = lane + 64 * i, px = id / CPP, ch = id - px * CPP;
        const u32x4 t = *reinterpret_cast<const u32x4*>(so + px * OS + ch * 8);
        const int mm = m0 + w * 32 + px, n = o0 + ch * 8;
        if (mm < M && n < O) *reinterpret_cast<u32x4*>(out + (size_t)mm * (size_t)ldo + n) = t;
    }
}

inline bool d1_dims_ok(int M, int K, int N, int act) {
    return M >= 1 && K >= 8 && N >= 8 && K <= D1_MAXC && N <= D1_MAXC && (K % 8) == 0 && (N % 8) == 0 && (act == 0 || act == 1);
}

// one call: the operands of the GEMM OUT[M][O] = A'[M][R] . B[O][R]^T with their row pitches (elements)
struct D1Call {
    const bf16_t *a, *yin, *bm, *xin;
    const float *rt0, *rt1, *ot0, *ot1;
    bf16_t* out;
    int M, R, O, act, lda, ldyin, ldxin, ldo;
};

inline bool d1_ld_ok(int ld, int width) { return ld >= width && (ld % 8) == 0; }

template <int CT, bool BWD, bool ACC>
void d1_launch(const D1Call& c, int OT, hipStream_t s) {
    constexpr int BO = 32 * CT;
    constexpr size_t tiles = (size_t)(D1_BM + BO) * D1_LS * sizeof(bf16_t), trans = (size_t)4 * 32 * (BO + 8) * sizeof(bf16_t);
    constexpr size_t tab_off = tiles > trans ? tiles : trans;            // a multiple of 16 either way
    const int MT = (c.M + D1_BM - 1) / D1_BM, RP = (c.R + D1_BK - 1) / D1_BK * D1_BK;
    const size_t tabs = (size_t)(BWD ? 1 : 2) * RP * sizeof(float);
    // widest case (CT = 5, forward, R = 2048): 43008 B of transposed output + 16384 B of tables + 1280 B of static otab
    // = 60672 B of the 64 KiB a workgroup may have
    static_assert(tab_off % 16 == 0 && tab_off + 2 * D1_MAXC * sizeof(float) + 2 * BO * sizeof(float) <= 65536,
                  "tiles + reduction tables + otab must fit the 64 KiB of LDS a workgroup may have");
    hipLaunchKernelGGL((d1_kernel<CT, BWD, ACC>), dim3((unsigned)MT * (unsigned)OT), dim3(256), tab_off + tabs, s, c.a, c.yin,
                       c.bm, c.rt0, c.rt1, c.ot0, c.ot1, c.xin, c.out, c.M, c.R, c.O, c.act, MT, OT, (int)tab_off, c.lda,
                       c.ldyin, c.ldxin, c.ldo);
}

// fewest channel tiles of at most 160 channels that cover O, and the narrowest tile that does it
template <bool BWD, bool ACC>
void d1_dispatch(const D1Call& c, hipStream_t s) {
    const int OT = (c.O + 159) / 160, per = (c.O + OT - 1) / OT, ct = (per + 31) / 32;
    switch (ct) {
        case 1: d1_launch<1, BWD, ACC>(c, OT, s); break;
        case 2: d1_launch<2, BWD, ACC>(c, OT, s); break;
        case 3: d1_launch<3, BWD, ACC>(c, OT, s); break;
        case 4: d1_launch<4, BWD, ACC>(c, OT, s); break;
        default: d1_launch<5, BWD, ACC>(c, OT, s); break;
    }
}

}  // namespace

extern "C" int adil_dense1x1_fwd_ld(const void* x, int ldx, const float* pscale, const float* pshift, const void* w,
                                    const float* scale, const float* shift, void* y, int ldy, int M, int K, int N, int act,
                                    void* stream) {
    if (x == nullptr || pscale == nullptr || pshift == nullptr || w == nullptr || scale == nullptr || shift == nullptr ||
        y == nullptr || !d1_dims_ok(M, K, N, act) || !d1_ld_ok(ldx, K) || !d1_ld_ok(ldy, N))
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
        gx == nullptr || !d1_dims_ok(M, K, N, act) || !d1_ld_ok(ldg, N) || !d1_ld_ok(ldy, N) || !d1_ld_ok(ldxin, K) ||
        !d1_ld_ok(ldgx, K) || (accumulate != 0 && accumulate != 1))
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
