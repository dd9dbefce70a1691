"""float64 restatement of the pool-first transition kernels (csrc/adil_dense_transition.hip: adil_dense_transition_fwd /
adil_dense_transition_bwd), their operand generators, rows and premises, written over `classifier_reference.Arith` and
reusing tests/dense1x1_reference.py (imported, left as it is) for the prologue, D1Out, finish / expected, compare_exact and
gaussian_ratio.  Plain torch; CPU or GPU.

    prologue   pre = fadd(fmul(f32(x), pscale[k]), pshift[k])  (two fp32 roundings, no fma: dense1x1_reference.prologue);
               p = max(pre, 0) in fp32, <= 0 -> +0, NOT rounded
    pooling    pooled pixel (b, oh, ow) owns the input pixels p00 = (2oh, 2ow), p01 = (2oh, 2ow+1), p10 = (2oh+1, 2ow),
               p11 = (2oh+1, 2ow+1);  s = ((p00 + p01) + p10) + p11 in fp32, each add rounded;  a = bf16(s * 0.25)
    forward    y[Mo][N] = bf16(a[Mo][K] . w[N][K]^T)
    gradient   t = g[Mo][N] . wt[K][N]^T;  gx[pixel][k] = bf16((t * pscale[k]) * 0.25) where THAT pixel's pre > 0, else +0,
               for the four pixels of the window

The prologue and the pooling are specified operation by operation in fp32, so they are restated in fp32 on BOTH sides
(reference and emulation compute the very same pre, p, s, a and branches); everything behind them is written once over an
`Arith`.  Two kinds of legs:

exact legs    integer x, w, g, pscale from classifier_reference.SCALES (+-1/2, +-1, +-2), integer pshift.  Quantum,
              derived.  Forward: pre = x * pscale + pshift is a multiple of 1/2, exact in fp32, and so is p; s is a sum of
              four of them (below 2^13: exact), s * 0.25 a multiple of 1/8, and a = bf16(s * 0.25) is one too (rounding a
              multiple of 1/8 to 8 bits keeps it one); w is an integer, so a * w and every partial sum are multiples of
              1/8.  Gradient: t is an integer, times pscale a multiple of 1/2, times 1/4 a multiple of 1/8.  QUANTUM = 1/8
              both ways, and with sum |terms| < 2^23 quanta every value in ANY order is exact in fp32: the one correct
              output is the RNE bf16 rounding of the exact value and a kernel is compared BIT FOR BIT.  The premises are
              asserted on the reference alone (`reference_row`).
                clamp set     x in [-2, 2], pshift in [-1, 1]; on the even channels pshift = 0 and x = +-(1 | 2) sign(pscale)
                              with the sign taken from (window pixel j + k / 2) % 2, so on those channels every window
                              holds two kept and two clamped pixels: each branch of the ReLU holds >= 25 % of the elements
                              of p and >= 25 % of the (window, channel) pairs MIX kept and clamped pixels (both asserted);
                              pscale of both signs; w = +-1 with density min(1, 8 / K), g in [-3, 3].
                rounding set  |x| <= 511 (rounded to bf16, still integers), |pshift| <= 16, |w| <= 15 (3 beyond K = 128,
                              which keeps the premise at K = 2048), |g| <= 127: p needs up to 11 bits, so p, a and the
                              outputs are really rounded where the kernel rounds and nowhere else (asserted: >= 10 % of
                              the reference outputs are not bf16 values, forward and gradient).
gaussian leg  the operands of dense1x1_reference's gaussian leg (N(0,1), pscale from [0.5, 1.5] with random signs, the
              no-contraction channels k % 8 = 3 included: there pre is EXACTLY 0 for x = +c_k under the two specified
              roundings, so p = +0 and gx = +0, while one fma leaves the product's rounding residual).  `a` is the same on
              both sides, so the elementwise bound is, derived, not measured:
                  |out - r| <= 2^-8 |r| + A (1 + 2^-8),   A = acc_eps(S, n) = n 2^-24 S 2
              forward: n = K (K products, nothing behind them), S = |a| . |w|^T;  gradient: n = N + 1 (N products and the
              fp32 product by pscale; the product by 1/4 is exact), S = (|g| . |wt|^T) |pscale| / 4, r with the masks
              applied (they come from the xin handed in: the same on both sides).  No element is excluded.

Every operation is written once over an `Arith`: fp64 is the reference; fp32 with the reduction in chunks of 16 (the
kernel's MFMA step) is the CPU emulation of the kernel, which also takes the mutants of tests/test_dense_transition_cpu.py;
`unrounded` restates the whole function in fp64 without any rounding, for the comparison with torch's own operators."""
import functools
from typing import NamedTuple

import torch

import dense1x1_reference as d1
from classifier_reference import BF16, F32, F64, SCALES, Arith, bf16_rne, rng  # noqa: F401

QUANTUM = 0.125

# (B, H, W, K, N): one pooled pixel; pooled rows of 3 (the window must follow W, not the linear pixel index); image
# boundaries inside a tile with K a multiple of neither 16 nor 64 and N no multiple of 32; exactly one 128-pixel pooled
# tile; a tile tail at the network's first transition width; two channel tiles; 16 reduction chunks and four channel tiles;
# the widest K; five images of one pooled pixel with four gradient channel tiles; 1156 pooled pixels (ten pixel tiles: eight
# dealt round-robin to the XCDs, two in plain order) with two channel tiles of 96, forward (N = 192) and gradient (K = 192)
ROWS = [(1, 2, 2, 8, 8), (1, 2, 6, 24, 40), (3, 4, 6, 72, 136), (2, 16, 16, 96, 128), (2, 16, 18, 256, 128),
        (1, 14, 14, 512, 256), (1, 6, 6, 1024, 512), (1, 2, 2, 2048, 8), (5, 2, 2, 8, 512),
        (1, 68, 68, 24, 192), (1, 68, 68, 192, 24)]
# the exact leg of each row: the two sets alternate down the table
EXACT_LEG = {row: ("clamp", "rounding")[i % 2] for i, row in enumerate(ROWS)}
NEW_SYMBOLS = {"adil_dense_transition_fwd": 11, "adil_dense_transition_bwd": 13}
# the three transitions of DenseNet-121 at 224 x 224: (H = W of the input, K, N)
NETWORK_TRANSITIONS = [(56, 256, 128), (28, 512, 256), (14, 1024, 512)]


def row_name(B, H, W, K, N):
    return f"tr-B{B}-H{H}-W{W}-K{K}-N{N}"


def legs_of(row):
    return (EXACT_LEG[row], "gaussian")


def windows(B, H, W, linear=False):
    """[Mo][4] input pixel rows (p00, p01, p10, p11) of every pooled pixel, both in channels_last linear order.  linear:
    the mutant whose window is the pixels 4 mo .. 4 mo + 3 of the linear index."""
    mo = torch.arange(B * (H // 2) * (W // 2))
    if linear:
        return 4 * mo[:, None] + torch.arange(4)[None, :]
    wo = W // 2
    r, ow = mo // wo, mo % wo                                          # r = b * Ho + oh, and b H W + 2 oh W = 2 W r
    p00 = 2 * r * W + 2 * ow
    return torch.stack([p00, p00 + 1, p00 + W, p00 + W + 1], 1)


def pooled(ar, x, pscale, pshift, idx):
    """(pre [Min][K], s [Mo][K], a [Mo][K]): the prologue and the pooling as specified, in fp32 (fp64 and unrounded with
    `unrounded`).  Mutants: fma (dense1x1_reference.prologue), pool_bf16, no_quarter."""
    if "unrounded" in ar.mut:
        pre = x.double() * pscale.double() + pshift.double()
    else:
        pre = d1.prologue(ar, x, pscale, pshift)[0]
    p = torch.where(pre > 0, pre, torch.zeros_like(pre))
    if "pool_bf16" in ar.mut:                                          # mutant: p rounded to bf16 before the sum
        p = bf16_rne(p)
    s = ((p[idx[:, 0]] + p[idx[:, 1]]) + p[idx[:, 2]]) + p[idx[:, 3]]
    q = s if "no_quarter" in ar.mut else s * 0.25                      # mutant: the quarter dropped
    return pre, s, (q if "unrounded" in ar.mut else ar.rnd(q))


def _rnd(ar, v):
    return v if "unrounded" in ar.mut else ar.rnd(v)


def tr_fwd(ar, dims, x, pscale, pshift, w):
    """x [B H W][K], w [N][K] -> D1Out of y [Mo][N]."""
    B, H, W, K, N = dims
    dt = ar.dtype
    wd = w.to(dt)
    if "conv_first" in ar.mut:                                         # mutant: today's path, conv at full resolution,
        a = d1.prologue(ar, x, pscale, pshift)[1].to(dt)               # y rounded to bf16, then pooled
        y = ar.rnd(ar.mm(a, wd.t()))
        idx = windows(B, H, W)
        pre = (((y[idx[:, 0]] + y[idx[:, 1]]) + y[idx[:, 2]]) + y[idx[:, 3]]) * 0.25
        return d1.D1Out(pre, None, K)
    idx = windows(B, H, W, "linear_window" in ar.mut)
    a = pooled(ar, x, pscale, pshift, idx)[2].to(dt)
    acc = ar.mm(*d1._k_tail(ar, a, wd.t()))
    S = a.abs() @ wd.abs().t() if ar.ref else None
    return d1.D1Out(acc, S, K)


def tr_bwd(ar, dims, g, wt, xin, pscale, pshift):
    """g [Mo][N], wt [K][N], xin [B H W][K] -> D1Out of gx [B H W][K]."""
    B, H, W, K, N = dims
    dt = ar.dtype
    idx = windows(B, H, W, "linear_window" in ar.mut)
    wd, ps = wt.to(dt), pscale.to(dt)
    t = ar.mm(*d1._k_tail(ar, g.to(dt), wd.t()))
    v = t * ps if "no_quarter" in ar.mut else (t * ps) * 0.25
    pre_x, s, _ = pooled(ar, xin, pscale, pshift, idx)
    keep = pre_x > 0                                                   # each input pixel's own branch
    if "pooled_mask" in ar.mut:                                        # mutant: one mask per window, from s > 0
        keep = torch.zeros_like(keep)
        for j in range(4):
            keep[idx[:, j]] = s > 0
    pre = torch.zeros(B * H * W, K, dtype=dt)
    S = torch.zeros(B * H * W, K, dtype=dt) if ar.ref else None
    Sv = (g.to(dt).abs() @ wd.abs().t()) * ps.abs() * 0.25 if ar.ref else None
    for j in range(4):
        pre[idx[:, j]] = v
        if ar.ref:
            S[idx[:, j]] = Sv
    return d1.D1Out(pre, S, N + 1, False, keep)


# ---------------------------------------------------------------------------------------------------------- operands
class Operands(NamedTuple):
    x: torch.Tensor              # [B H W][K] bf16
    pscale: torch.Tensor         # [K] fp32
    pshift: torch.Tensor         # [K] fp32
    w: torch.Tensor              # [N][K] bf16
    wt: torch.Tensor             # [K][N] bf16, the transpose
    g: torch.Tensor              # [Mo][N] bf16


def operands(name, leg, dims):
    """leg: 'clamp' / 'rounding' (exact sets) or 'gaussian'.  On the CPU; the GPU tests copy the very same tensors."""
    B, H, W, K, N = dims
    Min, Mo = B * H * W, B * (H // 2) * (W // 2)
    if leg == "gaussian":
        o = d1.operands(name, leg, Min, K, N)
        return Operands(o.x, o.pscale, o.pshift, o.w, o.wt, o.g[:Mo].contiguous())
    gen = rng(name, leg)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen)
    pick = lambda n: torch.tensor(SCALES)[torch.randint(0, len(SCALES), (n,), generator=gen)]
    kk = torch.arange(K)
    pscale = pick(K)
    if leg == "clamp":
        x, g = ri(-2, 2, Min, K).float(), ri(-3, 3, Mo, N).float()
        pshift = ri(-1, 1, K).float()
        pscale[0], pscale[1] = 0.5, -2.0                               # both signs at every K
        even = kk % 2 == 0
        pshift[even] = 0.0
        idx = windows(B, H, W)
        amp = ri(1, 2, Min, K).float()
        for j in range(4):                                             # window pixel j keeps channel k iff (j + k / 2) even
            sign = torch.where((j + kk // 2) % 2 == 0, 1.0, -1.0) * pscale.sign()
            rows = idx[:, j]
            x[rows] = torch.where(even, amp[rows] * sign, x[rows])
        keep = torch.rand(N, K, generator=gen) < min(1.0, 8.0 / K)
        w = ((ri(0, 1, N, K) * 2 - 1) * keep).float()
    else:
        x, g = ri(-511, 511, Min, K).float(), ri(-127, 127, Mo, N).float()
        pshift = ri(-16, 16, K).float()
        wa = 15 if K <= 128 else 3
        w = ri(-wa, wa, N, K).float()
    w = w.to(BF16)
    return Operands(x.to(BF16), pscale.to(F32).contiguous(), pshift.to(F32).contiguous(), w.contiguous(), w.t().contiguous(),
                    g.to(BF16))


# ---------------------------------------------------------------------------------------------------------- premises
def assert_premise(name, o, leg):
    """Exact legs, on the reference alone: every value a multiple of the quantum, sum |terms| < 2^23 quanta; rounding set:
    at least 10 % of the outputs are not bf16 values."""
    worst = float(o.S.max()) / QUANTUM
    assert worst < 2.0 ** 23, f"{name}: sum |terms| = {worst:.0f} quanta >= 2^23: the exact leg's premise fails"
    assert bool((o.pre / QUANTUM == (o.pre / QUANTUM).round()).all()), f"{name}: the reference is no multiple of the quantum"
    r = d1.expected(o)
    inexact = float((bf16_rne(r) != r).double().mean())
    if leg == "rounding":
        assert inexact >= 0.10, f"{name}: only {inexact:.3f} of the outputs test the rounding"
    return worst, inexact


def clamp_shares(dims, ops):
    """(share of p <= 0, share of p > 0, share of (window, channel) pairs that mix kept and clamped pixels)."""
    B, H, W, K, N = dims
    pre = pooled(Arith(), ops.x, ops.pscale, ops.pshift, windows(B, H, W))[0]
    kept = pre > 0
    idx = windows(B, H, W)
    cnt = sum(kept[idx[:, j]].long() for j in range(4))
    lo, hi = d1.branch_shares(pre)
    return lo, hi, float(((cnt > 0) & (cnt < 4)).double().mean())


class Row(NamedTuple):
    dims: tuple
    ops: Operands
    fwd: d1.D1Out                # reference forward
    bwd: d1.D1Out                # reference gradient


@functools.lru_cache(maxsize=None)
def reference_row(dims, leg):
    """Operands and fp64 reference of one row of one leg, computed once and shared; never modified.  The premises of the
    exact legs are asserted on the reference alone."""
    name = row_name(*dims)
    ops, ref = operands(name, leg, dims), Arith()
    fwd = tr_fwd(ref, dims, ops.x, ops.pscale, ops.pshift, ops.w)
    bwd = tr_bwd(ref, dims, ops.g, ops.wt, ops.x, ops.pscale, ops.pshift)
    if leg != "gaussian":
        assert_premise(name + "/fwd", fwd, leg)
        assert_premise(name + "/bwd", bwd, leg)
        pre, s, _ = pooled(ref, ops.x, ops.pscale, ops.pshift, windows(*dims[:3]))
        assert bool((pre * 2 == (pre * 2).round()).all()) and float(s.abs().max()) < 2.0 ** 13, name
    if leg == "clamp":
        lo, hi, mixed = clamp_shares(dims, ops)
        assert min(lo, hi) >= 0.25, f"{name}: ReLU branch shares {lo:.3f} / {hi:.3f}"
        assert mixed >= 0.25, f"{name}: only {mixed:.3f} of the windows mix kept and clamped pixels"
        assert bool((ops.pscale > 0).any()) and bool((ops.pscale < 0).any()), f"{name}: pscale has one sign only"
    return Row(dims, ops, fwd, bwd)


def emulate(dims, leg, mut=()):
    """(reference Row, the fp32 emulation's y, its gx): fp32 arithmetic, reduction in chunks of 16."""
    r = reference_row(dims, leg)
    em, o = Arith(F32, 16, mut), r.ops
    y = d1.finish(em, tr_fwd(em, dims, o.x, o.pscale, o.pshift, o.w))
    gx = d1.finish(em, tr_bwd(em, dims, o.g, o.wt, o.x, o.pscale, o.pshift))
    return r, y, gx
