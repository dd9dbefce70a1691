"""float64 restatement of the pre-activated pointwise kernels (csrc/adil_dense1x1.hip: adil_dense1x1_fwd / adil_dense1x1_bwd),
their operand generators and comparators, written over `classifier_reference.Arith` in the manner of
pointwise8_reference.py.  Plain torch; CPU or GPU.

    prologue   pre = fadd(fmul(f32(x), pscale[k]), pshift[k])  (two fp32 roundings, no fma);  a = bf16(max(pre, 0)), <= 0 -> +0
    forward    y[M][N]  = act((a[M][K] . w[N][K]^T) * scale[n] + shift[n]),  act = max(., 0) (ReLU, not ReLU6) or identity
    gradient   gz = bf16(g * scale[n]) [& y > 0];  t = gz . wt^T, wt [K][N];  gx[M][K] = bf16(t * pscale[k]) where pre > 0, else +0

The prologue is specified operation by operation in fp32, so it is restated in fp32 on BOTH sides (reference and emulation
compute the very same `pre`, `a` and branch); everything behind it is written once over an `Arith`.  Two legs:

exact leg     integer x, w, g, scales AND pscales from classifier_reference.SCALES (+-1/2, +-1, +-2), integer shifts and
              pshifts.  Quantum, derived: pre = x * pscale + pshift is a multiple of 1/2 of at most 9 significant bits,
              exact in fp32, and a = bf16(max(pre, 0)) is a multiple of 1/2 (rounding a multiple of 1/2 to 8 bits keeps it
              one); a * w is a multiple of 1/2, so is every partial sum; times scale: a multiple of 1/4; plus an integer: a
              multiple of 1/4.  Gradient: g * scale is g times a power of two, exact in bf16; gz * wt and every partial sum
              are multiples of 1/2; times pscale: a multiple of 1/4.  QUANTUM = 1/4 for both directions, and with
              sum |terms| < 2^23 quanta every value in ANY order is exact in fp32: the one correct output is the RNE bf16
              rounding of the exact value and a kernel is compared BIT FOR BIT.  The premise is asserted on the reference
              alone.
                clamp set     act = 1: x in [-2, 2], pscale of both signs, pshift in [-1, 1]; the channels k % 4 = 0 / 1 of
                              the first pixel are set to pre = +|pscale| / -|pscale| (pshift 0 there), so each branch of
                              the prologue ReLU holds >= 25 % of the elements of `a` even in a row of 8; w = +-1 with
                              density min(1, 8 / K), integer shifts that centre the even / odd output channels of the first
                              pixel at -2 / +3, so each branch of the output ReLU holds >= 5 % of the outputs, in a row of
                              8 outputs too; g in [-3, 3].  The gradient's masks are these two (y is the forward's own
                              output, xin its input).  All shares are asserted on the reference alone.
                rounding set  act = 0: |x| <= 63, |pshift| <= 16, |w| <= 15, |g| <= 127: `a` and the outputs need more
                              than 8 bits, so RNE itself is tested (asserted: >= 10 % of the reference outputs are not bf16
                              values).
gaussian leg  N(0,1) operands, scales and pscales from [0.5, 1.5] with random signs.  `a` is the same on both sides (fp32
              restatement), so the elementwise bound is that of pointwise8_reference.py with this kernel's term counts,
              derived, not measured:
                  |out - r| <= 2^-8 |r| + A (1 + 2^-8),   A = acc_eps(S, n) = n 2^-24 S 2
              forward: n = K + 2 (K products, the scale, the shift), S = (|a| . |w|^T) |scale| + |shift|, r after the ReLU
              (1-Lipschitz); gradient: n = N + 1 (N products and the one fp32 product by pscale), S = (|gz| . |wt|^T)
              |pscale|, r with both masks applied (they come from the y and xin handed in: the same on both sides),
              restated from the ROUNDED gz.  A bounds the fp32 value before the one bf16 rounding, 2^-8 (|r| + A) that
              rounding.  No element is excluded.
              The channels k % 8 = 3 test the "no contraction" clause: x[m][k] = +-c_k and pshift[k] = -fl32(c_k pscale[k]),
              so pre is EXACTLY 0 (a = +0, gx = +0) for x = +c_k under the specified two roundings, while a single fma
              leaves the rounding residual of the product, positive for about half of the channels: gx != 0 where r = 0.

Every operation is written once over an `Arith`: fp64 is the reference; fp32 with the reduction in chunks of 16 (the
kernel's MFMA step) is the CPU emulation of the kernel, which also takes the mutants of tests/test_dense1x1_cpu.py."""
from typing import NamedTuple, Optional

import torch

from classifier_reference import BF16, CANARY, F32, F64, SCALES, Arith, acc_eps, bf16_rne, bits, rng  # noqa: F401
from pointwise8_reference import mask_source, round_gz  # noqa: F401  (the gradient's gz and the y handed to it)

QUANTUM = 0.25


def _layers():
    out, nf, h = [], 64, 56
    for i, n in enumerate((6, 12, 24, 16)):
        out += [(nf + 32 * j, 128, h, 1) for j in range(n)]
        nf += 32 * n
        if i != 3:
            out.append((nf, nf // 2, h, 0))
            nf //= 2
            h //= 2
    return out


# (K, N, H, act) of the 61 pre-activated 1x1 layers of DenseNet-121 at 224 x 224 in network order (H = W = grid of the
# layer's input; tests/test_dense1x1_cpu.py derives the list from the network itself): 58 dense layers (act 1: BatchNorm +
# ReLU behind the convolution) and 3 transitions (act 0)
DENSENET_LAYERS_ALL61 = _layers()
# the distinct (K, N, act) among them at the largest grid at which each occurs, in order of first appearance: K = 64 .. 992
# in steps of 32 with N = 128 (30 pairs) and the transitions 256 -> 128, 512 -> 256, 1024 -> 512.  That is 32 distinct
# (K, N) pairs; 256 -> 128 occurs with both acts (dense layer and transition), which makes 33 rows
DENSENET_SHAPES = []
for _k, _n, _h, _a in DENSENET_LAYERS_ALL61:
    if not any(s[0] == _k and s[1] == _n and s[3] == _a for s in DENSENET_SHAPES):
        DENSENET_SHAPES.append((_k, _n, _h, _a))

# (M, K, N, act) of the GPU table: every shape of the network at M = 200 with its act, then the edge rows: M in {1, 127,
# 128, 129, 300} (one pixel, around the 128-pixel tile, more than two tiles), K in {8, 24, 72, 96, 992, 2048} (no multiple
# of 16 / of 64, one chunk and many), N in {8, 40, 128, 136, 512} (no multiple of 32, one channel tile and many); every
# value once with act 1 and once with act 0.  The two rows at M = 1153 have ten pixel tiles and two channel tiles of 96,
# forward (N = 192) and gradient (K = 192): eight pixel tiles are dealt round-robin to the XCDs with their channel tiles,
# two keep the plain order
NETWORK_ROWS = [(200, k, n, a) for k, n, _, a in DENSENET_SHAPES]
EDGE_ROWS = [(1, 8, 8, 1), (127, 24, 40, 1), (128, 72, 128, 1), (129, 96, 136, 1), (300, 992, 512, 1), (129, 2048, 8, 1),
             (300, 8, 512, 0), (129, 24, 136, 0), (128, 2048, 128, 0), (127, 992, 40, 0), (1, 72, 8, 0), (300, 96, 40, 0),
             (1153, 24, 192, 1), (1153, 192, 24, 0)]
ROWS = NETWORK_ROWS + EDGE_ROWS
NAN_ROWS = [(129, 24, 40), (300, 200, 136)]


class D1Out(NamedTuple):
    pre: torch.Tensor                      # the value before the ReLU / the mask and the rounding
    S: Optional[torch.Tensor]              # sum |terms| of pre (reference only)
    n: int                                 # number of terms of pre
    relu: bool = False                     # max(., 0) before the rounding
    keep: Optional[torch.Tensor] = None    # gradient: [pre(xin) > 0]; False -> +0


def finish(ar, o):
    """The output tensor (values, in the arithmetic's dtype) of a D1Out; a clamped or masked value is +0.  A kept zero has
    its IEEE sign: a zero sum t (+0: the accumulators start at +0) times a negative pscale is -0.0, as the header's
    gx = bf16(t * pscale) says."""
    v = o.pre
    if o.relu:
        v = torch.where(v > 0, v, torch.zeros_like(v))
    v = ar.rnd(v)
    if o.keep is not None:
        v = torch.where(o.keep, v, torch.zeros_like(v))
    return v


def expected(o):
    """r of the gaussian bound: the fp64 output before its rounding."""
    r = o.pre.clamp_min(0.0) if o.relu else o.pre
    return r if o.keep is None else torch.where(o.keep, r, torch.zeros_like(r))


def prologue(ar, x, pscale, pshift):
    """(pre, a) in fp32, as specified: pre = fadd(fmul(f32(x), pscale), pshift), a = bf16(max(pre, 0)), <= 0 -> +0."""
    x32, ps, pb = ar.f32(x), ar.f32(pscale), ar.f32(pshift)           # fp32 registers (the real values over `Unrounded`)
    if "fma" in ar.mut:                                                # mutant: the prologue contracted to one fma
        pre = ar.f32(x32.double() * ps.double() + pb.double())
    elif "no_pshift" in ar.mut:                                        # mutant: pshift dropped
        pre = x32 * ps
    else:
        pre = x32 * ps + pb                                            # two fp32 operations, each rounded
    if "no_pre_relu" in ar.mut:                                        # mutant: the prologue ReLU is missing
        return pre, ar.rnd(pre)
    return pre, ar.rnd(torch.where(pre > 0, pre, torch.zeros_like(pre)))


def _k_tail(ar, a, b):
    """Mutant: the last R % 16 columns of the reduction are dropped."""
    r = a.shape[1]
    if "k_tail" in ar.mut and r % 16:
        return a[:, :r - r % 16], b[:r - r % 16]
    return a, b


def d1_fwd(ar, x, pscale, pshift, w, scale, shift, act=0):
    """x [M][K], pscale / pshift [K], w [N][K], scale / shift [N]."""
    dt = ar.dtype
    a = prologue(ar, x, pscale, pshift)[1].to(dt)
    wd, sc, sh = w.to(dt), scale.to(dt), shift.to(dt)
    acc = ar.mm(*_k_tail(ar, a, wd.t()))
    pre = acc * sc + sh
    S = (a.abs() @ wd.abs().t()) * sc.abs() + sh.abs() if ar.ref else None
    return D1Out(pre, S, x.shape[1] + 2, bool(act))


def d1_bwd(ar, g, y, scale, wt, xin, pscale, pshift, act=0):
    """g, y [M][N], scale [N], wt [K][N], xin [M][K], pscale / pshift [K]; y None without act."""
    dt = ar.dtype
    gz = round_gz(ar, g, scale).to(dt)
    if act:
        yd = y.to(dt)
        gz = torch.where(yd >= 0 if "ge_mask" in ar.mut else yd > 0, gz, torch.zeros_like(gz))
    wd, ps = wt.to(dt), pscale.to(dt)
    t = ar.mm(*_k_tail(ar, gz, wd.t()))
    keep = prologue(ar, xin, pscale, pshift)[0] > 0
    if "row_mask" in ar.mut:                                           # mutant: the mask of the next pixel row
        keep = torch.roll(keep, -1, 0)
    if "no_pre_mask" in ar.mut:                                        # mutant: no prologue mask
        keep = None
    pre = t if "no_pscale_bwd" in ar.mut else t * ps                   # mutant: the pscale factor is missing
    S = (gz.abs() @ wd.abs().t()) * ps.abs() if ar.ref else None
    return D1Out(pre, S, g.shape[1] + 1, False, keep)


# ---------------------------------------------------------------------------------------------------------- operands
class Operands(NamedTuple):
    x: torch.Tensor              # [M][K] bf16
    pscale: torch.Tensor         # [K] fp32
    pshift: torch.Tensor         # [K] fp32
    w: torch.Tensor              # [N][K] bf16
    wt: torch.Tensor             # [K][N] bf16, the transpose
    scale: torch.Tensor          # [N] fp32
    shift: torch.Tensor          # [N] fp32
    g: torch.Tensor              # [M][N] bf16


def operands(name, leg, M, K, N):
    """leg: 'clamp' / 'rounding' (exact sets) or 'gaussian'.  On the CPU; the GPU tests copy the very same tensors."""
    gen = rng(name, leg)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen)
    pick = lambda n: torch.tensor(SCALES)[torch.randint(0, len(SCALES), (n,), generator=gen)]
    kk = torch.arange(K)
    if leg == "clamp":
        x, g = ri(-2, 2, M, K).float(), ri(-3, 3, M, N)
        pscale, pshift = pick(K), ri(-1, 1, K).float()
        pscale[0], pscale[1] = 0.5, -2.0                               # both signs at every K
        # the first pixel's channels k % 4 = 0 / 1: pre = +|pscale| / -|pscale|, a quarter of the row in each branch
        pshift[kk % 4 < 2] = 0.0
        x[0] = torch.where(kk % 4 == 0, pscale.sign(), torch.where(kk % 4 == 1, -pscale.sign(), x[0]))
        keep = torch.rand(N, K, generator=gen) < min(1.0, 8.0 / K)
        w = ((ri(0, 1, N, K) * 2 - 1) * keep).float()
        scale = pick(N)
        # integer shifts that put the FIRST pixel's even / odd channels at -2 / +3 (plus the fraction its product with the
        # scale may carry): one output per branch even in a row of 8 outputs; the other pixels spread around them
        pre0 = x[0] * pscale + pshift
        a0 = torch.where(pre0 > 0, pre0, torch.zeros_like(pre0)).double()
        acc0 = (a0 @ w.double().t()) * scale.double()
        shift = torch.tensor([-2.0, 3.0], dtype=F64)[torch.arange(N) % 2] - acc0.floor()
    elif leg == "rounding":
        x, g = ri(-63, 63, M, K).float(), ri(-127, 127, M, N)
        pscale, pshift = pick(K), ri(-16, 16, K).float()
        w = ri(-15, 15, N, K).float()
        scale, shift = pick(N), ri(-64, 64, N)
    else:
        rn = lambda *shape: torch.randn(shape, generator=gen)
        x, g = rn(M, K).to(BF16).float(), rn(M, N)
        pscale = ((0.5 + torch.rand(K, generator=gen)) * (ri(0, 1, K) * 2 - 1)).to(F32)
        pshift = rn(K).to(F32) * 0.5
        # the contraction channels k % 8 = 3: x = +-c, pshift = -fl32(c * pscale): pre is exactly 0 for x = +c
        c = (0.5 + torch.rand(K, generator=gen)).to(BF16).float()
        sgn = (ri(0, 1, M, K) * 2 - 1).float()
        hit = kk % 8 == 3
        x = torch.where(hit, sgn * c, x)
        pshift = torch.where(hit, -(c * pscale), pshift)
        w = rn(N, K) * (3.0 / K ** 0.5)
        scale = (0.5 + torch.rand(N, generator=gen)) * (ri(0, 1, N) * 2 - 1)
        shift = rn(N)
    w = w.to(BF16)
    return Operands(x.to(BF16), pscale.to(F32).contiguous(), pshift.to(F32).contiguous(), w.contiguous(), w.t().contiguous(),
                    scale.to(F32).contiguous(), shift.to(F32).contiguous(), g.to(BF16))


# ---------------------------------------------------------------------------------------------------------- comparators
def assert_premise(name, o, leg):
    """Exact legs, on the reference alone: every value a multiple of the quantum, sum |terms| < 2^23 quanta; rounding set:
    at least 10 % of the outputs are not bf16 values."""
    worst = float(o.S.max()) / QUANTUM
    assert worst < 2.0 ** 23, f"{name}: sum |terms| = {worst:.0f} quanta >= 2^23: the exact leg's premise fails"
    assert bool((o.pre / QUANTUM == (o.pre / QUANTUM).round()).all()), f"{name}: the reference is no multiple of the quantum"
    r = expected(o)
    inexact = float((bf16_rne(r) != r).double().mean())
    if leg == "rounding":
        assert inexact >= 0.10, f"{name}: only {inexact:.3f} of the outputs test the rounding"
    return worst, inexact


def branch_shares(v):
    """Shares of v <= 0 and v > 0 (v: a pre-activation, or the stored y of the gradient's mask)."""
    pos = int((v > 0).sum())
    return (v.numel() - pos) / v.numel(), pos / v.numel()


def assert_clamp_set(name, ops, fwd, y):
    """Clamp set, on the reference alone: both branches of the prologue ReLU hold >= 20 % of `a` (the gradient's prologue
    mask is the same tensor), both branches of the output ReLU >= 5 % of the outputs, and so does the gradient's mask from
    the y handed in; pscale takes both signs."""
    pre = prologue(Arith(), ops.x, ops.pscale, ops.pshift)[0]
    sp, so, sy = branch_shares(pre), branch_shares(fwd.pre), branch_shares(y.double())
    assert min(sp) >= 0.20, f"{name}: prologue branch shares {sp}"
    assert min(so) >= 0.05, f"{name}: output branch shares {so}"
    assert min(sy) >= 0.05, f"{name}: gradient mask shares {sy}"
    assert bool((ops.pscale > 0).any()) and bool((ops.pscale < 0).any()), f"{name}: pscale has one sign only"
    return sp, so, sy


def compare_exact(name, got, o):
    """got: the kernel's (or emulation's) tensor; o: the reference D1Out.  Raises on any bit that differs (+0 and -0.0
    differ)."""
    want = finish(Arith(), o)
    got = got.reshape(want.shape)
    a, b = bits(got.cpu()), bits(want.cpu())
    if torch.equal(a, b):
        return 0
    bad = (a != b)
    first = tuple(int(v) for v in bad.nonzero()[0])
    raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} outputs differ in bits; first at [m][c] = {first}: "
                         f"got {float(got[first])}, want {float(want[first])} (exact {float(o.pre[first])})")


def gaussian_ratio(got, o):
    """max over elements of |got - r| / (2^-8 |r| + A (1 + 2^-8))."""
    r = expected(o)
    a = acc_eps(o.S, o.n)
    bound = (2.0 ** -8 * (r.abs() + a) + a).clamp_min(2.0 ** -126)
    return float(((got.reshape(r.shape).double().to(r.device) - r).abs() / bound).max())


class Row(NamedTuple):
    ops: Operands
    fwd: D1Out                   # reference forward
    y: Optional[torch.Tensor]    # the y handed to the gradient (None with act 0)
    bwd: D1Out                   # reference gradient


def reference_row(name, leg, M, K, N, act):
    """Operands and fp64 reference of one row of one leg, with the premises of the exact legs asserted."""
    ops, ref = operands(name, leg, M, K, N), Arith()
    fwd = d1_fwd(ref, ops.x, ops.pscale, ops.pshift, ops.w, ops.scale, ops.shift, act)
    y = mask_source(name, leg, finish(ref, fwd)) if act else None
    bwd = d1_bwd(ref, ops.g, y, ops.scale, ops.wt, ops.x, ops.pscale, ops.pshift, act)
    if leg != "gaussian":
        assert_premise(name + "/fwd", fwd, leg)
        assert_premise(name + "/bwd", bwd, leg)
    if leg == "clamp":
        assert_clamp_set(name, ops, fwd, y)
    return Row(ops, fwd, y, bwd)


def row_name(M, K, N, act):
    return f"d1-M{M}-K{K}-N{N}-act{act}"


def legs_of(act):
    """The exact set that goes with an act, and the gaussian leg."""
    return ("clamp" if act else "rounding", "gaussian")
