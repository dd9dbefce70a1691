// adil_attention.hip — whole-head self-attention of the frozen ViT-B/16, forward and input gradient, head dimension 64:
// adil_attn_fwd / adil_attn_bwd / adil_attn_max_tokens (include/adil_hip.h).  The operands keep the layouts of the two
// linear layers around the attention: qkv / gqkv [B][T][3][H][64], o / go [B][T][H][64] bf16, lse [B][H][T] fp32.
//
// One workgroup (512 threads, 8 waves) per (image, head); T <= 256 tokens are 25 to 32 KiB per operand, so a head's whole
// K and V (forward) or Q, K, V and dO (backward) sit in LDS as [Tp][AT_LS] bf16 images (Tp = T rounded up to 32, rows
// T .. Tp-1 are ZEROS; row stride 144 B: the 16-byte row reads are conflict-free, the transposed reads 2-way).  Each image
// is read by rows (ds_read_b128: an operand that is summed over d) and by ds_read_b64_tr_b16 (an operand that is summed
// over the token index), there is no second, transposed copy.  One barrier, behind the staging; the images are read-only
// after it.  No score matrix ever reaches memory.
//
// Every score tile is computed so that the index the NEXT product sums over lies on the accumulator's registers and the
// other one on the lane: the tile then is that product's B operand after a conversion to bf16 in place (registers
// 8s .. 8s+7 are k-step s; element j of lane half h is tile row 16s + 8(j>>2) + 4h + (j&3), and tr_frag() hands the other
// operand over in that same k order).  All second products have the form Y^T[d][.] = img^T[d][k] . X[k][.], so a lane
// ends with 4 consecutive d of ONE token per register group: 8-byte stores, and every per-token constant (1 / l, the
// scale) is a per-lane scalar.
//
//   attn_fwd_kernel   wave w owns queries 32w .. 32w+31 (Q fragments straight from global memory).  S^T = K Q^T for ALL key
//                     blocks into at most 8 accumulator tiles (128 registers), so the row maximum and the row sum are taken
//                     once, with no online rescaling: in-lane over the registers, then one exchange between the two lane
//                     halves.  O^T += V^T bf16(e); o = bf16(acc / l): an IEEE fp32 DIVISION on the accumulator, one
//                     rounding to bf16.  lse = m + logf(l).
//   attn_bwd_kernel   prologue: delta_i = sum_d f32(go) f32(o) while dO is staged (8 lanes per row, a fixed xor tree).
//                     Phase 1, wave w owns keys 32w ..: K and V fragments in registers, walks the query blocks with
//                     S = Q K^T and dP = dO V^T (query on the registers), gv^T += dO^T bf16(p), gk^T += Q^T bf16(ds).
//                     Phase 2, wave w owns queries 32w ..: Q and dO fragments in registers, walks the key blocks with
//                     S^T = K Q^T and dP^T = V dO^T (key on the registers), gq^T += K^T bf16(ds).  7 products per tile
//                     pair instead of 5, in exchange for no fp32 dQ image, no cross-wave sum and no atomics.
//                     p = exp(0.125 s - lse_i); ds = p (dp - delta_i) in fp32; gq and gk take the factor 0.125 on the fp32
//                     accumulator (exact), one rounding to bf16.
// exp is the hardware exp2 behind a multiplication with log2(e) (__expf).  Padding: p is SELECTED to zero where the key or
// the query index is >= T (never a product with a padded lse), padded image rows are zeros and the padded entries of the
// lse / delta vectors are zeros, so nothing undefined reaches a sum.  No load or store leaves the operands' extents;
// offsets are 64-bit; no atomics: the summation order is fixed by the decomposition, results are bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adil_common.h"
#include "adil_hip.h"
#include "adil_mfma.h"

namespace {

#define AT_D 64                        // head dimension
#define AT_LS 72                       // LDS row stride (elements): 144 B
#define AT_MAXT 256                    // 4 images of 256 x 144 B + two fp32 vectors = 146 KiB of the 160 KiB
#define AT_NBMAX (AT_MAXT / 32)
#define AT_THREADS 512
#define AT_SCALE 0.125f                // 1 / sqrt(64)

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4a __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.0f;
    return z;
}
// row of register r in a 32 x 32 accumulator tile, for lane half hh
__device__ __forceinline__ int crow(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// operand summed over d, k-step ks (d = 16 ks + 8 hh + j): 16 bytes of row row0 + (lane & 31)
__device__ __forceinline__ bf16x8 row_frag(const bf16_t* img, int row0, int ks, int lane) {
    return lds8(img + (row0 + (lane & 31)) * AT_LS + 16 * ks + 8 * (lane >> 5));
}
// A operand img^T[d = 32 dt + (lane & 31)][k], k = the 16 image rows rb .. rb+15 in the order of an accumulator tile's
// registers: element j of lane half hh is row rb + 8(j>>2) + 4hh + (j&3).  Two transposing reads of 4 rows x 16 columns per
// 16-lane group; every lane takes part (the callers branch wave-uniformly only).
__device__ __forceinline__ bf16x8 tr_frag(const bf16_t* img, int rb, int dt, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int li = lane & 15, g = lane >> 4;
    const bf16_t* a = img + (rb + 4 * (g >> 1) + (li >> 2)) * AT_LS + 32 * dt + 16 * (g & 1) + 4 * (li & 3);
    typedef bf16x4 __attribute__((address_space(3))) * lds_ptr;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)a);
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)(a + 8 * AT_LS));
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#else
    return bf16x8{};
#endif
}
// registers 8s .. 8s+7 of an accumulator tile as the bf16 B operand of k-step s
__device__ __forceinline__ bf16x8 acc_frag(const f32x16& x, int s) {
    u32x4 t;
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = pack2_bf16(x[8 * s + 2 * i], x[8 * s + 2 * i + 1]);
    return __builtin_bit_cast(bf16x8, t);
}
__device__ __forceinline__ bf16x8 zero_frag() { return __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u}); }

// rows 0 .. Tp-1 of one [T][64] operand (row pitch ld elements) into an LDS image, zeros behind row T-1
__device__ __forceinline__ void stage_image(bf16_t* img, const bf16_t* __restrict__ src, size_t ld, int T, int Tp, int tid) {
    for (int idx = tid; idx < Tp * 8; idx += AT_THREADS) {
        const int row = idx >> 3, ch = idx & 7;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (row < T) v = *reinterpret_cast<const u32x4*>(src + (size_t)row * ld + (size_t)(8 * ch));
        *reinterpret_cast<u32x4*>(img + row * AT_LS + 8 * ch) = v;
    }
}
// this lane's fragments of row row0 + (lane & 31) straight from global memory, zeros behind row T-1
__device__ __forceinline__ void global_frags(bf16x8 (&f)[4], const bf16_t* __restrict__ src, size_t ld, int row, int T, int hh) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) f[ks] = zero_frag();
    if (row < T) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) f[ks] = *reinterpret_cast<const bf16x8*>(src + (size_t)row * ld + (size_t)(16 * ks + 8 * hh));
    }
}
// acc^T tile pair (d on the registers, token (lane & 31) of block blk on the lane) -> dst rows, 8 bytes per register group
__device__ __forceinline__ void store_tiles(bf16_t* __restrict__ dst, size_t ld, const f32x16 (&acc)[2], float f, int tok, int T,
                                            int hh) {
    if (tok >= T) return;
    bf16_t* p = dst + (size_t)tok * ld;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const u32x2 t = {pack2_bf16(acc[dt][4 * g] * f, acc[dt][4 * g + 1] * f),
                             pack2_bf16(acc[dt][4 * g + 2] * f, acc[dt][4 * g + 3] * f)};
            *reinterpret_cast<u32x2*>(p + 32 * dt + 8 * g + 4 * hh) = t;
        }
}

__global__ __launch_bounds__(AT_THREADS) void attn_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ o,
                                                              float* __restrict__ lse, int T, int H) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int Tp = (T + 31) & ~31, NB = Tp >> 5;
    bf16_t* sk = reinterpret_cast<bf16_t*>(smem_raw);      // [Tp][AT_LS]
    bf16_t* sv = sk + Tp * AT_LS;                          // [Tp][AT_LS]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, hh = lane >> 5;
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const size_t HD = (size_t)H * AT_D, ld = 3 * HD;
    const bf16_t* q = qkv + (size_t)b * (size_t)T * ld + (size_t)h * AT_D;
    stage_image(sk, q + HD, ld, T, Tp, tid);
    stage_image(sv, q + 2 * HD, ld, T, Tp, tid);
    lds_sync();
    if (w >= NB) return;                                   // wave-uniform; no barrier follows

    const int qi = 32 * w + c;
    bf16x8 qf[4];
    global_frags(qf, q, ld, qi, T, hh);

    // S^T: key on the registers, query on the lane
    f32x16 s[AT_NBMAX];
    float m = -INFINITY;
#pragma unroll
    for (int jb = 0; jb < AT_NBMAX; ++jb) {
        if (jb < NB) {
            f32x16 acc = zero16();
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) mma16(acc, row_frag(sk, 32 * jb, ks, lane), qf[ks]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float t = 32 * jb + crow(r, hh) < T ? acc[r] * AT_SCALE : -INFINITY;
                acc[r] = t;
                m = fmaxf(m, t);
            }
            s[jb] = acc;
        }
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));                   // key 0 is real: m is a score
    float l = 0.0f;
#pragma unroll
    for (int jb = 0; jb < AT_NBMAX; ++jb) {
        if (jb < NB) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = __expf(s[jb][r] - m);      // exp2(-inf) = 0 for the padded keys
                s[jb][r] = e;
                l += e;
            }
        }
    }
    l += __shfl_xor(l, 32, 64);

    f32x16 ot[2] = {zero16(), zero16()};
#pragma unroll
    for (int jb = 0; jb < AT_NBMAX; ++jb) {
        if (jb < NB) {
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const bf16x8 pf = acc_frag(s[jb], st);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) mma16(ot[dt], tr_frag(sv, 32 * jb + 16 * st, dt, lane), pf);
            }
        }
    }
    if (qi < T) {
        bf16_t* p = o + ((size_t)b * (size_t)T + (size_t)qi) * HD + (size_t)h * AT_D;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const u32x2 t = {pack2_bf16(ot[dt][4 * g] / l, ot[dt][4 * g + 1] / l),
                                 pack2_bf16(ot[dt][4 * g + 2] / l, ot[dt][4 * g + 3] / l)};
                *reinterpret_cast<u32x2*>(p + 32 * dt + 8 * g + 4 * hh) = t;
            }
        if (hh == 0) lse[((size_t)b * (size_t)H + (size_t)h) * (size_t)T + (size_t)qi] = m + logf(l);
    }
}

__global__ __launch_bounds__(AT_THREADS) void attn_bwd_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o,
                                                              const float* __restrict__ lse, const bf16_t* __restrict__ go,
                                                              bf16_t* __restrict__ gqkv, int T, int H) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int Tp = (T + 31) & ~31, NB = Tp >> 5;
    bf16_t* sq = reinterpret_cast<bf16_t*>(smem_raw);      // four [Tp][AT_LS] images
    bf16_t* sk = sq + Tp * AT_LS;
    bf16_t* sv = sk + Tp * AT_LS;
    bf16_t* sg = sv + Tp * AT_LS;
    float* sl = reinterpret_cast<float*>(sg + Tp * AT_LS); // lse[Tp], delta[Tp]; zeros behind T-1
    float* sd = sl + Tp;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, hh = lane >> 5;
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const size_t HD = (size_t)H * AT_D, ld = 3 * HD;
    const size_t qoff = (size_t)b * (size_t)T * ld + (size_t)h * AT_D;
    const size_t ooff = (size_t)b * (size_t)T * HD + (size_t)h * AT_D;
    const bf16_t* q = qkv + qoff;
    stage_image(sq, q, ld, T, Tp, tid);
    stage_image(sk, q + HD, ld, T, Tp, tid);
    stage_image(sv, q + 2 * HD, ld, T, Tp, tid);
    // dO, and delta from the same loads: 8 lanes share a row, their partial sums meet in a fixed xor tree.  Tp * 8 is a
    // multiple of 256, so a wave is in the loop whole or not at all
    for (int idx = tid; idx < Tp * 8; idx += AT_THREADS) {
        const int row = idx >> 3, ch = idx & 7;
        u32x4 gv = {0u, 0u, 0u, 0u}, ov = {0u, 0u, 0u, 0u};
        if (row < T) {
            gv = *reinterpret_cast<const u32x4*>(go + ooff + (size_t)row * HD + (size_t)(8 * ch));
            ov = *reinterpret_cast<const u32x4*>(o + ooff + (size_t)row * HD + (size_t)(8 * ch));
        }
        *reinterpret_cast<u32x4*>(sg + row * AT_LS + 8 * ch) = gv;
        float gf[8], of[8];
        unpack8(gv, gf);
        unpack8(ov, of);
        float d = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d = fmaf(gf[e], of[e], d);
        d += __shfl_xor(d, 1, 64);
        d += __shfl_xor(d, 2, 64);
        d += __shfl_xor(d, 4, 64);
        if (ch == 0) sd[row] = d;
    }
    for (int i = tid; i < Tp; i += AT_THREADS)
        sl[i] = i < T ? lse[((size_t)b * (size_t)H + (size_t)h) * (size_t)T + (size_t)i] : 0.0f;
    lds_sync();
    if (w >= NB) return;                                   // wave-uniform; no barrier follows
    const int tok = 32 * w + c;                            // this lane's key (phase 1) and query (phase 2)

    {   // ---- phase 1: gk, gv of key block w; query on the registers, key on the lane
        bf16x8 kf[4], vf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kf[ks] = row_frag(sk, 32 * w, ks, lane);
            vf[ks] = row_frag(sv, 32 * w, ks, lane);
        }
        f32x16 gvt[2] = {zero16(), zero16()}, gkt[2] = {zero16(), zero16()};
        for (int ib = 0; ib < NB; ++ib) {
            f32x16 sa = zero16(), dp = zero16();
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                mma16(sa, row_frag(sq, 32 * ib, ks, lane), kf[ks]);
                mma16(dp, row_frag(sg, 32 * ib, ks, lane), vf[ks]);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i0 = 32 * ib + 8 * g + 4 * hh;
                const f32x4a lv = *reinterpret_cast<const f32x4a*>(sl + i0), dv = *reinterpret_cast<const f32x4a*>(sd + i0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g + e;
                    const float p = (i0 + e < T && tok < T) ? __expf(sa[r] * AT_SCALE - lv[e]) : 0.0f;
                    sa[r] = p;
                    dp[r] = p * (dp[r] - dv[e]);
                }
            }
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const bf16x8 pf = acc_frag(sa, st), df = acc_frag(dp, st);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    mma16(gvt[dt], tr_frag(sg, 32 * ib + 16 * st, dt, lane), pf);
                    mma16(gkt[dt], tr_frag(sq, 32 * ib + 16 * st, dt, lane), df);
                }
            }
        }
        store_tiles(gqkv + qoff + HD, ld, gkt, AT_SCALE, tok, T, hh);
        store_tiles(gqkv + qoff + 2 * HD, ld, gvt, 1.0f, tok, T, hh);
    }
    {   // ---- phase 2: gq of query block w; key on the registers, query on the lane
        bf16x8 qf[4], gf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qf[ks] = row_frag(sq, 32 * w, ks, lane);
            gf[ks] = row_frag(sg, 32 * w, ks, lane);
        }
        const float li = sl[tok], di = sd[tok];
        f32x16 gqt[2] = {zero16(), zero16()};
        for (int jb = 0; jb < NB; ++jb) {
            f32x16 sa = zero16(), dp = zero16();
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                mma16(sa, row_frag(sk, 32 * jb, ks, lane), qf[ks]);
                mma16(dp, row_frag(sv, 32 * jb, ks, lane), gf[ks]);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = (32 * jb + crow(r, hh) < T && tok < T) ? __expf(sa[r] * AT_SCALE - li) : 0.0f;
                dp[r] = p * (dp[r] - di);
            }
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const bf16x8 df = acc_frag(dp, st);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) mma16(gqt[dt], tr_frag(sk, 32 * jb + 16 * st, dt, lane), df);
            }
        }
        store_tiles(gqkv + qoff, ld, gqt, AT_SCALE, tok, T, hh);
    }
}

inline size_t attn_lds_fwd(int T) { return (size_t)2 * round_up(T, 32) * AT_LS * sizeof(bf16_t); }
inline size_t attn_lds_bwd(int T) { return (size_t)round_up(T, 32) * (4 * AT_LS * sizeof(bf16_t) + 2 * sizeof(float)); }
static_assert((size_t)AT_MAXT * (4 * AT_LS * sizeof(bf16_t) + 2 * sizeof(float)) <= 160 * 1024, "the backward images must fit the LDS of a CU");

inline bool attn_args_ok(int B, int T, int H) {
    // blockIdx.x carries (image, head)
    return B >= 1 && H >= 1 && T >= 1 && T <= AT_MAXT && (long long)B * (long long)H <= 2147483647LL;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------ //
extern "C" int adil_attn_max_tokens(void) { return AT_MAXT; }

extern "C" int adil_attn_fwd(const void* qkv, void* o, float* lse, int B, int T, int H, void* stream) {
    if (!qkv || !o || !lse || !attn_args_ok(B, T, H)) return ADIL_EINVAL;
    if (!aligned(qkv, 16) || !aligned(o, 16) || !aligned(lse, 16)) return ADIL_EINVAL;
    ADIL_ENTER();
    const size_t lds = attn_lds_fwd(T);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)attn_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(attn_fwd_kernel, dim3((unsigned)B * (unsigned)H), dim3(AT_THREADS), lds, (hipStream_t)stream,
                       (const bf16_t*)qkv, (bf16_t*)o, lse, T, H);
    ADIL_CHECK_LAUNCH();
    return 0;
}

extern "C" int adil_attn_bwd(const void* qkv, const void* o, const float* lse, const void* go, void* gqkv, int B, int T, int H,
                             void* stream) {
    if (!qkv || !o || !lse || !go || !gqkv || !attn_args_ok(B, T, H)) return ADIL_EINVAL;
    if (!aligned(qkv, 16) || !aligned(o, 16) || !aligned(lse, 16) || !aligned(go, 16) || !aligned(gqkv, 16)) return ADIL_EINVAL;
    ADIL_ENTER();
    const size_t lds = attn_lds_bwd(T);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)attn_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(attn_bwd_kernel, dim3((unsigned)B * (unsigned)H), dim3(AT_THREADS), lds, (hipStream_t)stream,
                       (const bf16_t*)qkv, (const bf16_t*)o, lse, (const bf16_t*)go, (bf16_t*)gqkv, T, H);
    ADIL_CHECK_LAUNCH();
    return 0;
}
