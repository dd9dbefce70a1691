// Experiment (not product): where do the 140 - 210 us of conv3x3_kernel's step loop (LOOP = 1, the parent of the unrolled
// loop) go at the four stride-1 shapes of ResNet-50, B = 512?  The kernel body is repeated here with phases that can be
// switched off at compile time; timing only — the ablated variants compute garbage.  The product kernels under both
// loops are timed next to them.  Input and output rotate over enough buffers (1 GB of them at least) that no launch
// finds its operands in the Infinity Cache.  Build + run (GPU box):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I dl_attack_on_imagenet_amd/csrc tools/exp/ablate_conv3x3.hip -o tools/exp/bin/ablate_conv3x3
//   tools/exp/bin/ablate_conv3x3 [launches per timing = 40] [shape 0..3, default all]
#include "../../dl_attack_on_imagenet_amd/csrc/adil_convs.hip"
#include <cstdio>
#include <cstdlib>
#include <vector>

enum { NO_WADDR = 1,     // weight loads from one address per thread, computed once (no per-tap 64-bit index arithmetic)
       NO_MASK = 2,      // no tap masks on the fragments
       NO_WSTAGE = 4,    // store_w off: the weight tile in LDS is never replaced
       NO_BARRIER = 8,   // no barrier per tap
       READ_AHEAD = 16,  // the fragments of ks + 1 are read before the MFMAs of ks (no wait on a read issued just before)
       NO_MFMA = 32,     // an xor on the fragments instead of the MFMAs
       NO_WLOAD = 64,    // no global weight loads after the prologue
       NO_XRELOAD = 128, // the halo of the first channel chunk stays (no global loads / LDS writes for later chunks)
       NO_READS = 256 }; // no LDS fragment reads: the MFMAs run on registers

template <int BN, int WPX, int ABL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void ablate_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp, bf16_t* __restrict__ y, int M, int H, int W, int C, int N,
    int MT, int NT) {
    constexpr int C3_BM = WPX * 64;
    constexpr int CTW = BN / 32 / (4 / WPX);
    constexpr int XCHK = (C3_BM + 128) * 8 / 256;
    constexpr int WCH = BN * 8 / 256;
    constexpr int OS = BN + 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int NP = C3_BM + 2 * W + 2;
    bf16_t* sx = reinterpret_cast<bf16_t*>(smem_raw);
    const int sx_elems = (NP * C3_LS > C3_BM * OS ? NP * C3_LS : C3_BM * OS);
    bf16_t* sw = sx + ((sx_elems + 7) & ~7);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int wpx = w % WPX, wch = w / WPX;
    int mt, nt;
    if ((MT & 7) == 0) {
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        nt = j % NT;
        mt = (j / NT) * 8 + xcd;
    } else {
        nt = blockIdx.x % NT;
        mt = blockIdx.x / NT;
    }
    const int m0 = mt * C3_BM, n0 = nt * BN;
    const int nci = C >> 6;
    int pl[2];
    unsigned vmask[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        pl[p] = (wpx * 2 + p) * 32 + c;
        const int m = m0 + pl[p];
        const int ww = m % W, hh = (m / W) % H;
        unsigned vm = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int kh = t / 3, kw = t - 3 * kh;
            const bool ok = (m < M) && (hh + kh - 1 >= 0) && (hh + kh - 1 < H) && (ww + kw - 1 >= 0) && (ww + kw - 1 < W);
            vm |= ok ? (1u << t) : 0u;
        }
        vmask[p] = vm;
    }
    u32x4 xr[XCHK], wr[3][WCH];
    auto load_x = [&](int cc) {
#pragma unroll
        for (int i = 0; i < XCHK; ++i) {
            const int q = tid + 256 * i, px = q >> 3, ch = q & 7;
            int gm = m0 - W - 1 + (px < NP ? px : NP - 1);
            gm = gm < 0 ? 0 : (gm >= M ? M - 1 : gm);
            xr[i] = *reinterpret_cast<const u32x4*>(x + (size_t)gm * C + cc * 64 + ch * 8);
        }
    };
    auto store_x = [&]() {
#pragma unroll
        for (int i = 0; i < XCHK; ++i) {
            const int q = tid + 256 * i, px = q >> 3, ch = q & 7;
            if (px < NP) *reinterpret_cast<u32x4*>(sx + px * C3_LS + ch * 8) = xr[i];
        }
    };
    const int nit = nci * 9;
    const bf16_t* wfix[WCH];                                          // NO_WADDR: tile 0's addresses, computed once
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
        const int q = tid + 256 * i, row = q >> 3, ch = q & 7;
        wfix[i] = wp + ((size_t)(n0 + row) * 9) * C + ch * 8;
    }
    auto load_w = [&](int it, u32x4 (&r)[WCH]) {
        if constexpr (ABL & NO_WADDR) {
#pragma unroll
            for (int i = 0; i < WCH; ++i) r[i] = *reinterpret_cast<const u32x4*>(wfix[i]);
        } else {
            const int itc = it < nit ? it : nit - 1;
            const int cc = itc / 9, tap = itc - 9 * cc;
#pragma unroll
            for (int i = 0; i < WCH; ++i) {
                const int q = tid + 256 * i, row = q >> 3, ch = q & 7;
                r[i] = *reinterpret_cast<const u32x4*>(wp + ((size_t)(n0 + row) * 9 + tap) * C + cc * 64 + ch * 8);
            }
        }
    };
    auto store_w = [&](int buf, const u32x4 (&r)[WCH]) {
#pragma unroll
        for (int i = 0; i < WCH; ++i) {
            const int q = tid + 256 * i, row = q >> 3, ch = q & 7;
            *reinterpret_cast<u32x4*>(sw + (buf * BN + row) * C3_LS + ch * 8) = r[i];
        }
    };
    auto barrier = [&]() __attribute__((always_inline)) { if constexpr (!(ABL & NO_BARRIER)) lds_barrier(); };

    f32x16 acc[2][CTW];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[p][ct][r] = 0.0f;
    struct Frag {
        bf16x8 b0, b1, a[CTW];
    };
    auto tap_body = [&](int it, u32x4 (&rfree)[WCH], const u32x4 (&rnext)[WCH]) {
        const int buf = it & 1;
        const int cc = it / 9, tap = it - 9 * cc;
        const int kh = tap / 3, kw = tap - 3 * kh;
        if constexpr (!(ABL & NO_WLOAD)) load_w(it + 3, rfree);
        if constexpr (!(ABL & NO_XRELOAD)) {
            if (tap == 4 && cc + 1 < nci) load_x(cc + 1);
        }
        const bf16_t* bw = sw + (buf * BN + (wch * CTW) * 32 + c) * C3_LS + 8 * h;
        const int shift = kh * W + kw;
        const bool ok0 = (vmask[0] >> tap) & 1u, ok1 = (vmask[1] >> tap) & 1u;
        auto read = [&](Frag& f, int ks) __attribute__((always_inline)) {
            if constexpr (ABL & NO_READS) {
                f.b0 = __builtin_bit_cast(bf16x8, rnext[0]);
                f.b1 = __builtin_bit_cast(bf16x8, rnext[WCH - 1]);
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) f.a[ct] = __builtin_bit_cast(bf16x8, xr[ct]);
            } else {
                f.b0 = lds8(sx + (pl[0] + shift) * C3_LS + 16 * ks + 8 * h);
                f.b1 = lds8(sx + (pl[1] + shift) * C3_LS + 16 * ks + 8 * h);
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) f.a[ct] = lds8(bw + ct * 32 * C3_LS + 16 * ks);
            }
        };
        auto mul = [&](Frag& f, int ks) __attribute__((always_inline)) {
            if constexpr (!(ABL & NO_MASK)) {
                u32x4 z0 = __builtin_bit_cast(u32x4, f.b0), z1 = __builtin_bit_cast(u32x4, f.b1);
#pragma unroll
                for (int j = 0; j < 4; ++j) { z0[j] = ok0 ? z0[j] : 0u; z1[j] = ok1 ? z1[j] : 0u; }
                f.b0 = __builtin_bit_cast(bf16x8, z0);
                f.b1 = __builtin_bit_cast(bf16x8, z1);
            }
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct) {
                if constexpr (ABL & NO_MFMA) {
                    const unsigned a0 = __builtin_bit_cast(u32x4, f.a[ct])[0];
                    acc[0][ct][ks] += __uint_as_float(a0 ^ __builtin_bit_cast(u32x4, f.b0)[ks]);
                    acc[1][ct][ks] += __uint_as_float(a0 ^ __builtin_bit_cast(u32x4, f.b1)[ks]);
                } else {
                    mma16(acc[0][ct], f.a[ct], f.b0);
                    mma16(acc[1][ct], f.a[ct], f.b1);
                }
            }
        };
        if constexpr (ABL & READ_AHEAD) {
            Frag f[2];
            read(f[0], 0);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                if (ks < 3) read(f[(ks + 1) & 1], ks + 1);
                __builtin_amdgcn_sched_barrier(0);
                mul(f[ks & 1], ks);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                Frag f;
                read(f, ks);
                mul(f, ks);
            }
        }
        if constexpr (!(ABL & NO_WSTAGE)) {
            if (it + 1 < nit) store_w(buf ^ 1, rnext);
        }
        if constexpr (!(ABL & NO_XRELOAD)) {
            if (tap == 8 && cc + 1 < nci) {
                barrier();
                store_x();
            }
        }
        barrier();
    };

    load_x(0);
    load_w(0, wr[0]);
    load_w(1, wr[1]);
    load_w(2, wr[2]);
    store_x();
    store_w(0, wr[0]);
    store_w(1, wr[1]);                                                // both buffers hold data whatever is switched off
    __syncthreads();
    for (int it = 0; it < nit; it += 3) {
        tap_body(it, wr[0], wr[1]);
        tap_body(it + 1, wr[1], wr[2]);
        tap_body(it + 2, wr[2], wr[0]);
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                u32x2 t;
                t[0] = pack2_bf16(acc[p][ct][4 * q], acc[p][ct][4 * q + 1]);
                t[1] = pack2_bf16(acc[p][ct][4 * q + 2], acc[p][ct][4 * q + 3]);
                *reinterpret_cast<u32x2*>(sx + pl[p] * OS + (wch * CTW + ct) * 32 + 8 * q + 4 * h) = t;
            }
        }
    }
    __syncthreads();
    constexpr int CPP = BN / 8;
#pragma unroll
    for (int i = 0; i < C3_BM * CPP / 256; ++i) {
        const int id = tid + 256 * i, px = id / CPP, ch = id - px * CPP;
        const int mm = m0 + px;
        if (mm < M) *reinterpret_cast<u32x4*>(y + (size_t)mm * N + n0 + ch * 8) = *reinterpret_cast<const u32x4*>(sx + px * OS + ch * 8);
    }
}

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(r_), __LINE__); exit(1); } } while (0)

struct Ctx {
    int B = 512, H, W, C, M, MT, NT;
    std::vector<bf16_t*> x, y;
    bf16_t* wp;
    hipEvent_t e0, e1;
    size_t lds;
};

template <typename K>
static void time_kernel(Ctx& c, K kernel, size_t lds, const char* name, int rep) {
    CK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    auto launch = [&](int i) {
        const size_t j = i % c.x.size();
        hipLaunchKernelGGL(kernel, dim3((unsigned)(c.MT * c.NT)), dim3(256), lds, 0, (const bf16_t*)c.x[j], (const bf16_t*)c.wp,
                           c.y[j], c.M, c.H, c.W, c.C, c.C, c.MT, c.NT);
    };
    for (int i = 0; i < 4; ++i) launch(i);
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(c.e0));
    for (int i = 0; i < rep; ++i) launch(i);
    CK(hipEventRecord(c.e1));
    CK(hipEventSynchronize(c.e1));
    float ms;
    CK(hipEventElapsedTime(&ms, c.e0, c.e1));
    printf("| %-100s | %6.1f us |\n", name, ms * 1e3 / rep);
    fflush(stdout);
}

template <int BN, int WPX, int ABL>
static void run(Ctx& c, const char* name, int rep) { time_kernel(c, ablate_kernel<BN, WPX, ABL>, c.lds, name, rep); }

template <int BN, int WPX>
static void shape(int H, int C, int rep) {
    Ctx c;
    c.H = c.W = H;
    c.C = C;
    c.M = c.B * H * H;
    constexpr int BM = WPX * 64;
    c.MT = (c.M + BM - 1) / BM;
    c.NT = C / BN;
    const int NP = BM + 2 * c.W + 2;
    size_t sx_elems = (size_t)NP * C3_LS;
    if (sx_elems < (size_t)BM * (BN + 8)) sx_elems = (size_t)BM * (BN + 8);
    sx_elems = (sx_elems + 7) & ~(size_t)7;
    c.lds = (sx_elems + (size_t)2 * BN * C3_LS) * sizeof(bf16_t);
    const size_t n = (size_t)c.M * C;
    const size_t nbuf = ((size_t)1 << 30) / (4 * n) + 2;             // x and y: 4 bytes per element and buffer pair
    c.x.resize(nbuf);
    c.y.resize(nbuf);
    for (auto& p : c.x) { CK(hipMalloc(&p, n * 2)); CK(hipMemset(p, 0x3c, n * 2)); }
    for (auto& p : c.y) { CK(hipMalloc(&p, n * 2)); }
    CK(hipMalloc(&c.wp, (size_t)9 * C * C * 2)); CK(hipMemset(c.wp, 0x3c, (size_t)9 * C * C * 2));
    CK(hipEventCreate(&c.e0)); CK(hipEventCreate(&c.e1));
    printf("\nconv3x3_kernel<%d, %d> ablation, 512 x %d x %d x %d -> %d: %d x %d workgroups, LDS %zu B, %zu buffer pairs\n\n", BN, WPX,
           H, H, C, C, c.MT, c.NT, c.lds, nbuf);
    printf("| variant | time |\n|---|---|\n");
    for (int pass = 0; pass < 2; ++pass) {
        time_kernel(c, conv3x3_kernel<BN, WPX, 1>, c.lds, "product kernel, step loop (LOOP = 1)", rep);
        time_kernel(c, conv3x3_kernel<BN, WPX, 0>, c.lds + C3_LS * sizeof(bf16_t), "product kernel, unrolled taps and pipelined reads (LOOP = 0)", rep);
        run<BN, WPX, 0>(c, "the step loop repeated here, nothing switched off", rep);
        run<BN, WPX, NO_WADDR>(c, "without the weight-address arithmetic (one address per thread)", rep);
        run<BN, WPX, NO_MASK>(c, "without the tap masks", rep);
        run<BN, WPX, NO_WADDR | NO_MASK>(c, "without both", rep);
        run<BN, WPX, NO_WSTAGE>(c, "without the weight staging (store_w off)", rep);
        run<BN, WPX, NO_WLOAD | NO_WSTAGE>(c, "without weight loads and staging", rep);
        run<BN, WPX, NO_XRELOAD>(c, "without the halo reload of later chunks", rep);
        run<BN, WPX, NO_BARRIER>(c, "without the barrier per tap", rep);
        run<BN, WPX, READ_AHEAD>(c, "LDS reads one ks ahead", rep);
        run<BN, WPX, READ_AHEAD | NO_WADDR | NO_MASK>(c, "LDS reads one ks ahead, no address arithmetic, no masks", rep);
        run<BN, WPX, READ_AHEAD | NO_WADDR | NO_MASK | NO_BARRIER>(c, "the same without the barrier", rep);
        run<BN, WPX, NO_READS>(c, "without the LDS fragment reads (MFMAs on registers)", rep);
        run<BN, WPX, NO_MFMA>(c, "without the MFMAs", rep);
        run<BN, WPX, NO_MFMA | NO_READS | NO_MASK>(c, "stream only: global loads, LDS writes, barriers, stores", rep);
        run<BN, WPX, NO_WLOAD | NO_WSTAGE | NO_XRELOAD | NO_BARRIER | NO_MASK | NO_READS>(c, "MFMAs only", rep);
    }
    for (auto p : c.x) CK(hipFree(p));
    for (auto p : c.y) CK(hipFree(p));
    CK(hipFree(c.wp));
}

int main(int argc, char** argv) {
    const int rep = argc > 1 ? atoi(argv[1]) : 40;
    const int only = argc > 2 ? atoi(argv[2]) : -1;
    if (only < 0 || only == 0) shape<64, 4>(56, 64, rep);
    if (only < 0 || only == 1) shape<128, 2>(28, 128, rep);
    if (only < 0 || only == 2) shape<128, 2>(14, 256, rep);
    if (only < 0 || only == 3) shape<128, 2>(7, 512, rep);
    return 0;
}
