// adil_pw_tile.h — the GEMM tile shared by the narrow pointwise kernels: pw8_kernel (adil_pointwise8.hip), d1_kernel
// (adil_dense1x1.hip), tr_fwd_kernel and tr_bwd_kernel (adil_dense_transition.hip).  d3_kernel (adil_dense3x3.hip) takes
// pw_tile_order from here and nothing else: its tile is another one.
//
// All of them are the row-major GEMM  OUT[M][O] = A'[M][R] . B[O][R]^T  (M = pixels, R and O multiples of 8, not of 64) and
// all are HBM streams: what matters is that an activation crosses HBM once, in 16-byte accesses.
//   Workgroup = 4 waves = 128 pixels x BO output channels, BO = 32 CT with CT = 1 .. 5 picked on the host (pw_dispatch) so
//   that the fewest channel tiles cover O: one tile up to O = 160, so every narrow layer reads its input once.
//   The reduction runs in chunks of 64 through LDS (row stride 72), the next chunk waiting in registers, in MFMA steps of
//   16; only the steps the chunk holds are issued (R = 16 is one step).
//   MFMA roles as in adil_convs.hip: A operand = B rows (channels -> accumulator registers), B operand = pixels -> lanes;
//   a lane owns 4 consecutive channels of one pixel per register quad; the finished tile goes through a per-wave LDS
//   transpose (pw_stage) to 16-byte stores (pw_write_out).
//   Tails are clipped and zero-filled, never read from a neighbour: a 16-byte chunk past R (R % 8 == 0: a chunk is wholly
//   inside or wholly outside) and a B row past O are read at a clamped in-range address and replaced by zeros on BOTH
//   operands (0 x NaN would be NaN); a pixel row past M reads row M - 1 and is not stored.
// What a kernel keeps in its own file: how the A operand is formed on the way from registers to LDS (its load_tiles /
// store_tiles), the epilogue arithmetic, and where its per-channel tables live.
// A piece is shared where every instantiation keeps its registers, LDS and occupancy (profiles/pw_tile_refactor.md).  hipcc
// optimises a __forceinline__ helper on its own before it inlines it, so a helper is no textual paste; where a piece moved a
// register count of pw8_kernel or d1_kernel (or, pw_stage in d1_kernel, its time) it is written out there, under a comment
// that names the piece it restates.  A change to such a piece goes to those copies too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "adil_common.h"
#include "adil_mfma.h"

namespace {

constexpr int PW_BM = 128;                 // pixels of a workgroup
constexpr int PW_BK = 64;                  // reduction channels of a chunk
constexpr int PW_LS = PW_BK + 8;           // LDS row stride (elements): 144 B = 9 x 16 B
constexpr int PW_MAXC = 2048;              // most channels on either side
constexpr int PW_ACH = PW_BM * PW_BK / 8 / 256;      // 16-byte chunks of the A tile per thread (4)

// Workgroups are dealt round-robin to the 8 XCDs: the OT channel tiles of one pixel tile go to ONE XCD, so the repeated
// reads of an A tile (of a halo, in d3_kernel) meet in that XCD's L2.  Pixel tiles behind the last multiple of 8 keep the
// plain order.
__device__ __forceinline__ void pw_tile_order(int MT, int OT, int& mt, int& ot) {
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

// the pre-activation of one input element: the product and the sum are each rounded to fp32 (no contraction), so an
// fp32 restatement reproduces the value AND the branch pre > 0, in the forward and in the gradient alike.  The two
// operations are written out under the pragma, INSIDE the body: __fmul_rn / __fadd_rn are plain `*` and `+` in a header,
// outside the pragma's reach, and contract to one fma after inlining (FINDINGS.md 202)
__device__ __forceinline__ float pw_preact(float x, float ps, float pb) {
#pragma clang fp contract(off)
    const float p = x * ps;
    return p + pb;
}

// the accumulate form's value: the product is rounded to fp32 BEFORE the old gradient is added (no fma)
__device__ __forceinline__ float pw_mul_add(float t, float ps, float old) {
#pragma clang fp contract(off)
    const float v = t * ps;
    return old + v;
}

// The B tile [32 CT][64] of a kernel: where it comes from, the registers that hold the chunk ahead, where it goes.  The
// members are REFERENCES to the kernel's variables, which is what the captures of the kernels' load_tiles / store_tiles (the
// callers of load() and store()) are.  Passed by value the same code compiles differently: the helper is simplified alone
// first, the clamped load becomes an unconditional load plus selects and the LDS addresses lose their `inbounds`, 2 - 10
// VGPRs either way.
template <int CT>
struct PwBTile {
    u32x4 (&br)[CT];
    const bf16_t* __restrict const& bm;
    bf16_t* const& sb;
    const int &o0, &O, &R, &tid;

    // this thread's 16-byte column of reduction chunk kc, the same for every row of the thread and for the A tile too; past
    // R: cok is false and the column is clamped to 0
    __device__ __forceinline__ int column(int kc, bool& cok) const {
        const int col = kc * PW_BK + (tid & 7) * 8;
        cok = col < R;
        return cok ? col : 0;
    }
    // one chunk into registers: rows past O and columns past R (cok false) are zeros
    __device__ __forceinline__ void load(bool cok, int colc) const {
        const u32x4 zero4 = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < CT; ++i) {
            const int n = o0 + ((tid + 256 * i) >> 3);
            const bool ok = cok && n < O;
            br[i] = *reinterpret_cast<const u32x4*>(bm + (ok ? (size_t)n * (size_t)R + colc : (size_t)0));
            if (!ok) br[i] = zero4;
        }
    }
    __device__ __forceinline__ void store() const {
        const int ch = tid & 7;
#pragma unroll
        for (int i = 0; i < CT; ++i) {
            const int row = (tid + 256 * i) >> 3;
            *reinterpret_cast<u32x4*>(sb + row * PW_LS + ch * 8) = br[i];
        }
    }
};

template <int CT>
__device__ __forceinline__ void pw_clear(f32x16 (&acc)[CT]) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.0f;
}

// One chunk of the reduction, between the kernel's two lds_barrier() calls: acc += sa [128][PW_LS] . sb [32 CT][PW_LS]^T for
// this wave's 32 pixels; `left` = reduction channels from this chunk on, and only the MFMA steps the chunk holds are issued
template <int CT>
__device__ __forceinline__ void pw_mma_chunk(f32x16 (&acc)[CT], const bf16_t* sa, const bf16_t* sb, int left, int w, int c, int h) {
    const bf16_t* bx = sa + (w * 32 + c) * PW_LS + 8 * h;
    const bf16_t* bw = sb + c * PW_LS + 8 * h;
    const int steps = left >= PW_BK ? PW_BK / 16 : (left + 15) / 16;
    for (int ks = 0; ks < steps; ++ks) {
        const bf16x8 b = lds8(bx + 16 * ks);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) mma16(acc[ct], lds8(bw + ct * 32 * PW_LS + 16 * ks), b);
    }
}

// accumulators -> epilogue -> bf16 -> this wave's transposed buffer so [32][32 CT + 8] (the tile buffers, idle behind the
// reduction): lane = pixel c, register quad q of tile ct = channels co = 32ct + 8q + 4h .. +3.  epi(v, ct, q, co) is the
// kernel's own arithmetic on the four fp32 values; the rounding (RNE) is here.
template <int CT, class Epi>
__device__ __forceinline__ void pw_stage(const f32x16 (&acc)[CT], bf16_t* so, int c, int h, Epi&& epi) {
    constexpr int OS = 32 * CT + 8;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int co = 32 * ct + 8 * q + 4 * h;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[ct][4 * q + e];
            epi(v, ct, q, co);
            u32x2 t;
            t[0] = pack2_bf16(v[0], v[1]);
            t[1] = pack2_bf16(v[2], v[3]);
            *reinterpret_cast<u32x2*>(so + c * OS + co) = t;
        }
    }
}

// this wave's transposed buffer of the workgroup's
template <int CT>
__device__ __forceinline__ bf16_t* pw_stage_buffer(unsigned char* smem_raw, int w) {
    return reinterpret_cast<bf16_t*>(smem_raw) + w * 32 * (32 * CT + 8);
}

// the wave's staged 32 pixels x 32 CT channels to out (row pitch ldo, elements) in 16-byte stores
template <int CT>
__device__ __forceinline__ void pw_write_out(const bf16_t* so, bf16_t* out, int ldo, int m0, int o0, int M, int O,
                                             int w, int lane) {
    constexpr int OS = 32 * CT + 8, CPP = 32 * CT / 8;   // 16-byte chunks per pixel
#pragma unroll
    for (int i = 0; i < 32 * CPP / 64; ++i) {
        const int id = lane + 64 * i, px = id / CPP, ch = id - px * CPP;
        const u32x4 t = *reinterpret_cast<const u32x4*>(so + px * OS + ch * 8);
        const int mm = m0 + w * 32 + px, n = o0 + ch * 8;
        if (mm < M && n < O) *reinterpret_cast<u32x4*>(out + (size_t)mm * (size_t)ldo + n) = t;
    }
}

// ---- host side

// the GEMM's extents as every entry point needs them
inline bool pw_dims_ok(int M, int K, int N, int act) {
    return M >= 1 && K >= 8 && N >= 8 && K <= PW_MAXC && N <= PW_MAXC && (K % 8) == 0 && (N % 8) == 0 && (act == 0 || act == 1);
}

inline bool pw_ld_ok(int ld, int width) { return ld >= width && (ld % 8) == 0; }

inline int pw_pixel_tiles(int M) { return (M + PW_BM - 1) / PW_BM; }

// dynamic LDS of the tile: the A and B chunks, reused for the transposed output; a multiple of 16 either way
template <int CT>
constexpr size_t pw_tile_bytes() {
    constexpr int BO = 32 * CT;
    constexpr size_t tiles = (size_t)(PW_BM + BO) * PW_LS * sizeof(bf16_t), trans = (size_t)4 * 32 * (BO + 8) * sizeof(bf16_t);
    return tiles > trans ? tiles : trans;
}

// the run-time ct = 1 .. 5 (anything above: 5) as a type
template <int CT = 1, class F>
void pw_with_ct(int ct, int OT, F&& f) {
    if constexpr (CT == 5)
        f(std::integral_constant<int, 5>{}, OT);
    else if (ct == CT)
        f(std::integral_constant<int, CT>{}, OT);
    else
        pw_with_ct<CT + 1>(ct, OT, f);
}

// fewest channel tiles OT of at most 160 channels that cover O, and the narrowest tile CT that does it: calls
// f(std::integral_constant<int, CT>, OT)
template <class F>
void pw_dispatch(int O, F&& f) {
    const int OT = (O + 159) / 160, per = (O + OT - 1) / OT;
    pw_with_ct((per + 31) / 32, OT, f);
}

}  // namespace
