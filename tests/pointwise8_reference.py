"""float64 restatement of the narrow-channel pointwise kernels (csrc/adil_pointwise8.hip: adil_pw8_fwd / adil_pw8_bwd),
their operand generators and comparators, written over `classifier_reference.Arith`.  Plain torch; CPU or GPU.

    forward    y[M][N]  = act((x[M][K] . w[N][K]^T) * scale[n] + shift[n] (+ res[M][N])),  act = clamp to [0, 6] or identity
    gradient   gz = bf16(g * scale[n]) [& 0 < y < 6];  gx[M][K] = gz . wt^T,  wt [K][N]

The kernels multiply bf16 operands, accumulate in fp32 and round ONCE to bf16, to nearest even; ReLU6 clamps the fp32 value
before the rounding (0 and 6 are bf16 values and rounding is monotone, so the order does not show in the bits).  Two legs:

exact leg     integer operands, scales from classifier_reference.SCALES (+-1/2, +-1, +-2), integer shifts: every product,
              every partial sum in ANY order and every epilogue value is a multiple of the quantum 1/2 below 2^23 quanta,
              exact in fp32, so the one correct output is the RNE bf16 rounding of the exact value and a kernel is compared
              BIT FOR BIT.  The premise is asserted on the reference alone (sum |terms| < 2^23 quanta).
                clamp set     act = 1: x in [-2, 2], w = +-1 with density min(1, 8 / K) (else 0), g in [-3, 3], integer
                              shifts that centre the channels n % 3 = 0 / 1 / 2 of the first pixel in the three branches.
                              The accumulator has a standard deviation of 4 at every K, so each of the branches
                              pre <= 0, 0 < pre < 6, pre >= 6 holds at least 5 % of the outputs, in a row of 8 outputs
                              too, and so does the gradient's mask (both asserted).  The transposed weight has the same
                              density, so the gradient sums 8 N / K terms.
                rounding set  act = 0: |x| <= 127, |w| <= 15, |g| <= 127: outputs need more than 8 bits, so RNE itself is
                              tested (asserted: at least 10 % of the reference outputs are not bf16 values).
gaussian leg  N(0,1) operands, scales from [0.5, 1.5] with random signs; elementwise bound, derived, not measured:
                  |out - r| <= 2^-8 |r| + A (1 + 2^-8),   A = acc_eps(S, n) = n 2^-24 S 2
              forward: n = K + 2 (+ 1 with res), r after the clamp (1-Lipschitz); gradient: n = N, r with the mask applied
              (the mask comes from the y handed in: the same on both sides), restated from the ROUNDED gz (one fp32
              product, one rounding: no contraction can change it), so it carries one rounding term.  S = sum |terms|.
              No element is excluded.

Every operation is written once over an `Arith`: fp64 is the reference; fp32 with the reduction in chunks of 16 (the
kernel's MFMA step) is the CPU emulation of the kernel, which also takes the mutants of tests/test_pointwise8_cpu.py."""
from typing import NamedTuple, Optional

import torch

from classifier_reference import BF16, CANARY, F32, F64, SCALES, Arith, acc_eps, bf16_rne, bits, rng

QUANTUM = 0.5

# (K, N, H, act, res) of the 34 1x1 layers of MobileNetV2 at 224 x 224 in network order (H = W = grid of the layer;
# tests/test_pointwise8_cpu.py derives the list from the network itself): 16 expansions, 17 projections, the last layer
_E = lambda k, n, h: (k, n, h, 1, False)
_P = lambda k, n, h, res=False: (k, n, h, 0, res)
MOBILENET_LAYERS_ALL34 = [
    _P(32, 16, 112),
    _E(16, 96, 112), _P(96, 24, 56), _E(24, 144, 56), _P(144, 24, 56, True),
    _E(24, 144, 56), _P(144, 32, 28), _E(32, 192, 28), _P(192, 32, 28, True), _E(32, 192, 28), _P(192, 32, 28, True),
    _E(32, 192, 28), _P(192, 64, 14), _E(64, 384, 14), _P(384, 64, 14, True), _E(64, 384, 14), _P(384, 64, 14, True),
    _E(64, 384, 14), _P(384, 64, 14, True),
    _E(64, 384, 14), _P(384, 96, 14), _E(96, 576, 14), _P(576, 96, 14, True), _E(96, 576, 14), _P(576, 96, 14, True),
    _E(96, 576, 14), _P(576, 160, 7), _E(160, 960, 7), _P(960, 160, 7, True), _E(160, 960, 7), _P(960, 160, 7, True),
    _E(160, 960, 7), _P(960, 320, 7),
    _E(320, 1280, 7)]
# the 19 distinct (K, N, H) among them, in order of first appearance, with act and "some layer of this shape has a residual"
MOBILENET_SHAPES = []
for _k, _n, _h, _a, _r in MOBILENET_LAYERS_ALL34:
    _hit = [i for i, s in enumerate(MOBILENET_SHAPES) if s[:3] == (_k, _n, _h)]
    if _hit:
        MOBILENET_SHAPES[_hit[0]] = (_k, _n, _h, _a, MOBILENET_SHAPES[_hit[0]][4] or _r)
    else:
        MOBILENET_SHAPES.append((_k, _n, _h, _a, _r))

# (M, K, N, act, res) of the GPU table: the 19 (K, N) pairs at M = 200 with act / res as the network uses them, then the
# edge rows: M in {1, 127, 128, 129, 300} (one pixel, around the 128-pixel tile, more than two tiles), K in {8, 24, 72,
# 200, 2048} (no multiple of 16 / of 64, one chunk and many), N in {8, 24, 40, 136, 2048} (no multiple of 32, one channel
# tile and many); every value once with act 0 and once with act 1, two rows with res.  The two rows at M = 1153 have ten
# pixel tiles and two channel tiles of 96, forward (N = 192) and gradient (K = 192): eight pixel tiles are dealt round-robin
# to the XCDs with their channel tiles, two keep the plain order
NETWORK_ROWS = [(200, k, n, a, r) for k, n, _, a, r in MOBILENET_SHAPES]
EDGE_ROWS = [(1, 8, 8, 1, False), (127, 24, 24, 1, False), (128, 72, 40, 1, False), (129, 200, 136, 1, False),
             (300, 2048, 2048, 1, False),
             (300, 8, 2048, 0, False), (129, 24, 40, 0, True), (128, 200, 24, 0, False), (127, 2048, 136, 0, True),
             (1, 72, 8, 0, False),
             (1153, 24, 192, 1, False), (1153, 192, 24, 0, False)]
ROWS = NETWORK_ROWS + EDGE_ROWS
NAN_ROWS = [(129, 24, 40), (300, 200, 136)]


class P8Out(NamedTuple):
    pre: torch.Tensor                      # the value before the clamp and the rounding
    S: Optional[torch.Tensor]              # sum |terms| of pre (reference only)
    n: int                                 # number of terms of pre
    act: bool = False                      # clamp to [0, 6]
    unwritten: Optional[torch.Tensor] = None   # emulation of a mutant that leaves outputs unwritten (True there)


def clamp6(ar, v):
    if "no_clamp6" in ar.mut:                                          # mutant: the clamp at 6 is missing
        return v.clamp_min(0.0)
    return v.clamp(0.0, 6.0)


def finish(ar, o):
    """The output tensor (values, in the arithmetic's dtype) of a P8Out; a clamped non-positive value is +0."""
    v = clamp6(ar, o.pre) + 0.0 if o.act else o.pre
    v = ar.rnd(v)
    if o.unwritten is not None:
        v = torch.where(o.unwritten, torch.full_like(v, CANARY), v)
    return v


def expected(o):
    """r of the gaussian bound: the fp64 output before its rounding."""
    return o.pre.clamp(0.0, 6.0) if o.act else o.pre


def relu6_mask(ar, y):
    """[0 < y < 6] by value (-0.0 is a zero)."""
    lo = y >= 0 if "ge_mask" in ar.mut else y > 0
    if "no_lt6" in ar.mut:                                             # mutant: the mask's `< 6` is missing
        return lo
    return lo & (y < 6)


def _k_tail(ar, a, b):
    """Mutant: the last K % 16 columns of the reduction are dropped."""
    r = a.shape[1]
    if "k_tail" in ar.mut and r % 16:
        return a[:, :r - r % 16], b[:r - r % 16]
    return a, b


def pw8_fwd(ar, x, w, scale, shift, res=None, act=0):
    """x [M][K], w [N][K], scale / shift [N], res [M][N] or None."""
    dt = ar.dtype
    xd, wd, sc, sh = x.to(dt), w.to(dt), scale.to(dt), shift.to(dt)
    acc = ar.mm(*_k_tail(ar, xd, wd.t()))
    pre = acc * sc
    if "no_shift" not in ar.mut:
        pre = pre + sh
    S = (xd.abs() @ wd.abs().t()) * sc.abs() + sh.abs() if ar.ref else None
    if res is not None:
        if "no_res" not in ar.mut:
            pre = pre + res.to(dt)
        if ar.ref:
            S = S + res.to(dt).abs()
    unwritten = None
    n_out = w.shape[0]
    if "n_tail" in ar.mut and n_out % 32:                              # mutant: the last N % 32 channels stay unwritten
        unwritten = torch.zeros(pre.shape, dtype=torch.bool, device=pre.device)
        unwritten[:, n_out - n_out % 32:] = True
    return P8Out(pre + 0.0, S, x.shape[1] + 2 + (res is not None), bool(act), unwritten)


def round_gz(ar, g, scale):
    """bf16(g * scale) as the kernel forms it: one fp32 product, one rounding."""
    v = ar.f32(g) if "no_scale_bwd" in ar.mut else ar.f32(g) * ar.f32(scale)
    return ar.rnd(v)


def pw8_bwd(ar, g, y, scale, wt, act=0):
    """g, y [M][N], scale [N], wt [K][N]; y None without act."""
    dt = ar.dtype
    gz = round_gz(ar, g, scale).to(dt)
    if act:
        gz = torch.where(relu6_mask(ar, y.to(dt)), gz, torch.zeros_like(gz))
    wd = wt.to(dt)
    acc = ar.mm(*_k_tail(ar, gz, wd.t()))
    S = gz.abs() @ wd.abs().t() if ar.ref else None
    unwritten = None
    k_out = wt.shape[0]
    if "n_tail" in ar.mut and k_out % 32:
        unwritten = torch.zeros(acc.shape, dtype=torch.bool, device=acc.device)
        unwritten[:, k_out - k_out % 32:] = True
    return P8Out(acc + 0.0, S, g.shape[1], False, unwritten)


# ---------------------------------------------------------------------------------------------------------- operands
class Operands(NamedTuple):
    x: torch.Tensor              # [M][K] bf16
    w: torch.Tensor              # [N][K] bf16
    wt: torch.Tensor             # [K][N] bf16, the transpose
    scale: torch.Tensor          # [N] fp32
    shift: torch.Tensor          # [N] fp32
    res: Optional[torch.Tensor]  # [M][N] bf16
    g: torch.Tensor              # [M][N] bf16


def operands(name, leg, M, K, N, with_res=False):
    """leg: 'clamp' / 'rounding' (exact sets) or 'gaussian'.  On the CPU; the GPU tests copy the very same tensors."""
    gen = rng(name, leg)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen)
    pick = lambda n: torch.tensor(SCALES)[torch.randint(0, len(SCALES), (n,), generator=gen)]
    if leg == "clamp":
        x, g, r = ri(-2, 2, M, K), ri(-3, 3, M, N), ri(-3, 3, M, N)
        keep = torch.rand(N, K, generator=gen) < min(1.0, 8.0 / K)
        w = (ri(0, 1, N, K) * 2 - 1) * keep
        scale = pick(N)
        # integer shifts that put the FIRST pixel's channels n % 3 = 0 / 1 / 2 at -2 / 3 / 8 (plus the half its product with
        # the scale may carry): one output per branch even in a row of 8 outputs; the other pixels spread around them
        acc0 = (x[0].double() @ w.double().t()) * scale.double()
        shift = torch.tensor([-2.0, 3.0, 8.0], dtype=F64)[torch.arange(N) % 3] - acc0.floor()
    elif leg == "rounding":
        x, g, r = ri(-127, 127, M, K), ri(-127, 127, M, N), ri(-127, 127, M, N)
        w = ri(-15, 15, N, K)
        scale, shift = pick(N), ri(-64, 64, N)
    else:
        rn = lambda *shape: torch.randn(shape, generator=gen)
        x, g, r = rn(M, K), rn(M, N), rn(M, N)
        w = rn(N, K) * (3.0 / K ** 0.5)
        scale = (0.5 + torch.rand(N, generator=gen)) * (ri(0, 1, N) * 2 - 1)
        shift = rn(N)
    w = w.to(BF16)
    return Operands(x.to(BF16), w.contiguous(), w.t().contiguous(), scale.to(F32).contiguous(), shift.to(F32).contiguous(),
                    r.to(BF16) if with_res else None, g.to(BF16))


def mask_source(name, leg, y_ref):
    """The y handed to the gradient: the forward's own (reference) output, values 0 and 6 included; in the exact legs half
    of its zeros are turned into -0.0, which the kernel's value comparison must treat as the zero it is."""
    y = y_ref.to(BF16)
    if leg != "gaussian":
        flip = (torch.rand(y.shape, generator=rng(name, leg + "/negzero")) < 0.5) & (y == 0)
        y = torch.where(flip, torch.full_like(y, -0.0), y)
    return y


# ---------------------------------------------------------------------------------------------------------- comparators
def assert_premise(name, o, leg):
    """Exact legs, on the reference alone: every value a multiple of the quantum, sum |terms| < 2^23 quanta; rounding set:
    at least 10 % of the outputs are not bf16 values."""
    worst = float(o.S.max()) / QUANTUM
    assert worst < 2.0 ** 23, f"{name}: sum |terms| = {worst:.0f} quanta >= 2^23: the exact leg's premise fails"
    assert bool((o.pre / QUANTUM == (o.pre / QUANTUM).round()).all()), f"{name}: the reference is no multiple of the quantum"
    inexact = float((bf16_rne(o.pre) != o.pre).double().mean())
    if leg == "rounding":
        assert inexact >= 0.10, f"{name}: only {inexact:.3f} of the outputs test the rounding"
    return worst, inexact


def branch_shares(v):
    """Shares of v <= 0, 0 < v < 6, v >= 6 (v: a pre-activation, or the stored y of the gradient's mask)."""
    n = v.numel()
    lo, hi = int((v <= 0).sum()), int((v >= 6).sum())
    return lo / n, (n - lo - hi) / n, hi / n


def assert_branches(name, v, least=0.05):
    shares = branch_shares(v)
    assert min(shares) >= least, f"{name}: branch shares {shares}: one of the three ReLU6 branches is nearly empty"
    return shares


def compare_exact(name, got, o):
    """got: the kernel's (or emulation's) tensor; o: the reference P8Out.  Raises on any bit that differs (+0 and -0.0
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
