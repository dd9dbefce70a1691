"""float64 restatement of the first-convolution kernels (csrc/adil_first_conv.hip: adil_first3x3_fwd / adil_first3x3_bwd),
their operand generators and comparators, written over `classifier_reference.Arith`.  Plain torch; CPU or GPU.

    forward    x' = bf16(f32(f32(x - mean[c]) * inv_std[c])), zero padded AFTER the normalisation;
               y[b][oh][ow][n] = bf16(act((sum x'[b][c][2oh-1+kh][2ow-1+kw] w[n][c][kh][kw]) * scale[n] + shift[n]))
    gradient   gz = bf16(g * scale[n]) [& 0 < y < 6];
               gx[b][c][h][w] = round(inv_std[c] * sum gz[b][(h+1-kh)/2][(w+1-kw)/2][n] w[n][c][kh][kw])

x and gx are [B][3][H][W] (fp32 or bf16), y and g [B][OH][OW][32] bf16, w [32][3][3][3] bf16.  x' and gz are formed bit
exactly as the kernel forms them: fp32 operations, one rounding each, then bf16 to nearest even; everything after that is
fp64, rounded once where the kernel rounds.  Three operand sets:

exact legs    every product, every partial sum in ANY order and every epilogue value is a multiple of the quantum 1/4
              below 2^24 quanta, exact in fp32, so the one correct output is the rounding of the exact value and a kernel is
              compared BIT FOR BIT, the sign of zeros included.  The premise is asserted on the reference alone.
              x is on the integer grid, the mean is on the integer grid too — (1, 0, -1), not all zero: x - mean stays exact,
              and a zero mean would hide three of the mutants of tests/test_first_conv_cpu.py (the mean's sign, padding in
              raw-pixel space, and x' left unrounded on bf16 streams) — inv_std = (1, 1/2, 2), scales from
              classifier_reference.SCALES, shifts on the half-integer grid.
                clamp set     relu6 = 1: x in [-2, 2], w = +-1 with density 1/9 (else 0), g in [-3, 3]; the shifts centre the
                              channels n % 3 = 0 / 1 / 2 at -2 / 3 / 8, so that each of the branches y = 0, 0 < y < 6, y = 6
                              holds at least 5 % of the outputs, and so does the gradient's mask (both asserted).
                rounding set  relu6 = 0: |x| <= 600, |w| <= 15, |g| <= 127: x', y and gx need more than 8 bits, so the three
                              roundings themselves are tested (asserted: at least 10 % of the reference values of x' and of
                              y are not bf16 values, in rows of at least 96 input values).
gaussian leg  N(0,1) operands, the ImageNet mean and std, scales from [0.5, 1.5] with random signs.  Elementwise bound,
              derived, not measured.  The operands of both sums (x', gz, w) are the same bits on both sides, so the only
              errors are those of the fp32 accumulation and of the last rounding.  A sum of n fp32 terms with sum |terms| =
              S, accumulated in any order, is within n 2^-24 S of the exact sum (each of the n - 1 additions and each of the
              products' own roundings — none here: a product of two bf16 values is exact in fp32 — contributes at most
              2^-24 of a partial sum that is at most S); the epilogue's two operations (forward: * scale, + shift; gradient:
              * inv_std) add two more such terms, covered by the factor 2:  A = acc_eps(S, n) = n 2^-24 S 2.  A bf16 output
              adds half an ulp of the value it rounds, 2^-8 (|r| + A):
                  bf16 outputs   |out - r| <= 2^-8 |r| + A (1 + 2^-8)
                  fp32 gx        |out - r| <= A + 2^-24 |r|
              forward: n = 27, S = (sum |x'| |w|) |scale| + |shift|, r after the clamp (1-Lipschitz); gradient: n = 128 (at
              most 4 taps of 32 channels), S = inv_std sum |gz| |w|, r with the mask applied (the mask comes from the y
              handed in: the same on both sides).  No element is excluded.

Every operation is written once over an `Arith`: fp64 is the reference; fp32 with one partial sum per tap row (the
kernel's MFMA step) is the CPU emulation of the kernel, which also takes the mutants of tests/test_first_conv_cpu.py."""
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from classifier_reference import BF16, CANARY, F32, F64, SCALES, Arith, acc_eps, bf16_rne, bits, rng

QUANTUM = 0.25
COUT = 32
FWD_TILE = (16, 16)              # output tile (OH, OW) of first3x3_fwd
BWD_TILE = (16, 32)              # output tile (H, W) of first3x3_bwd
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EXACT_MEAN, EXACT_INV_STD = (1.0, 0.0, -1.0), (1.0, 0.5, 2.0)

# (B, H, W, x dtype, relu6).  The five small shapes; OH = 15 / 16 / 17 and OW = 15 / 16 / 17 around the forward tile; H = 15
# / 16 / 17 and W = 31 / 32 / 33 around the gradient tile; two images across a tile edge; one image at 224 x 224
ROWS = [(1, 1, 1, BF16, 1), (1, 2, 3, F32, 1), (3, 7, 9, BF16, 1), (2, 8, 8, F32, 1), (1, 33, 17, BF16, 1),
        (1, 29, 5, F32, 1), (1, 31, 6, BF16, 1), (1, 34, 4, F32, 1),
        (1, 5, 30, BF16, 1), (1, 6, 32, F32, 1), (1, 4, 33, BF16, 1),
        (1, 15, 31, F32, 1), (2, 16, 32, BF16, 1), (1, 17, 33, BF16, 0), (1, 17, 33, F32, 1),
        (1, 224, 224, BF16, 1)]
NAN_ROWS = [(1, 7, 9), (1, 33, 35)]


def out_grid(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


class FCOut(NamedTuple):
    pre: torch.Tensor                      # the value before the clamp and the rounding
    S: Optional[torch.Tensor]              # sum |terms| of pre (reference only)
    n: int                                 # number of terms of pre
    act: bool = False                      # clamp to [0, 6]
    dtype: torch.dtype = BF16              # storage type of the output


def finish(ar, o):
    """The output tensor (values, in the arithmetic's dtype) of an FCOut; a clamped non-positive value and a zero are +0."""
    v = o.pre.clamp(0.0, 6.0) + 0.0 if o.act else o.pre + 0.0
    v = ar.rnd(v) if o.dtype == BF16 else ar.f32(v).to(v.dtype)
    if "neg_zero" in ar.mut:                                           # mutant: -0.0 is emitted
        v = torch.where(v == 0, torch.full_like(v, -0.0), v)
    return v


def expected(o):
    """r of the gaussian bound: the fp64 output before its rounding."""
    return o.pre.clamp(0.0, 6.0) if o.act else o.pre


def _table(ar, v, like):
    """Three floats as the kernel receives them: fp32 arguments (`ar.f32`: the doubles themselves over `Unrounded`)."""
    return ar.f32(torch.tensor(v, dtype=F64, device=like.device)).view(1, 3, 1, 1)


def normalise(ar, x, mean, inv_std):
    """x' as the kernel forms it: two fp32 operations no contraction can merge, one rounding to bf16.  Unpadded."""
    m, s = _table(ar, mean, x), _table(ar, inv_std, x)
    d = ar.f32(x) + m if "mean_sign" in ar.mut else ar.f32(x) - m
    v = d * s
    return v if "no_round_x" in ar.mut else ar.rnd(v)


def first_fwd(ar, x, w, mean, inv_std, scale, shift, relu6=1):
    """x [B][3][H][W] fp32 / bf16, w [32][3][3][3], scale / shift [32] -> y [B][OH][OW][32]."""
    dt = ar.dtype
    B, _, H, W = x.shape
    OH, OW = out_grid(H, W)
    if "raw_pad" in ar.mut:                                            # mutant: the padding is applied in raw-pixel space
        xp = normalise(ar, F.pad(x.float(), (1, 1, 1, 1)), mean, inv_std).to(dt)
    else:
        xp = F.pad(normalise(ar, x, mean, inv_std).to(dt), (1, 1, 1, 1))
    wd = w.to(dt)
    if "chan_order" in ar.mut:                                         # mutant: the input channels are read in reverse order
        wd = wd.flip(1)
    acc = torch.zeros(B * OH * OW, COUT, dtype=dt, device=x.device)
    S = torch.zeros_like(acc) if ar.ref else None
    for kh in range(3):                                                # one partial sum per tap row: K order (kw, c)
        cols = torch.cat([xp[:, :, kh:kh + 2 * OH - 1:2, kw:kw + 2 * OW - 1:2].permute(0, 2, 3, 1).reshape(-1, 3)
                          for kw in range(3)], 1)
        wk = wd[:, :, kh].permute(0, 2, 1).reshape(COUT, 9)
        acc = acc + ar.mm(cols, wk.t())
        if ar.ref:
            S += cols.abs() @ wk.abs().t()
    sc, sh = scale.to(dt), shift.to(dt)
    pre = acc * sc + sh
    if ar.ref:
        S = S * sc.abs() + sh.abs()
    shape = (B, OH, OW, COUT)
    return FCOut(pre.reshape(shape) + 0.0, None if S is None else S.reshape(shape), 27, bool(relu6))


def round_gz(ar, g, scale):
    """bf16(g * scale) as the kernel forms it: one fp32 product, one rounding."""
    v = ar.f32(g) if "no_scale_bwd" in ar.mut else ar.f32(g) * ar.f32(scale)
    return ar.rnd(v)


def relu6_mask(ar, y):
    """[0 < y < 6] by value (-0.0 is a zero)."""
    lo = y >= 0 if "ge_mask" in ar.mut else y > 0
    hi = y <= 6 if "le_mask" in ar.mut else y < 6
    return lo & hi


def first_bwd(ar, g, y, scale, w, inv_std, H, W, relu6=1, out_dtype=BF16):
    """g, y [B][OH][OW][32] (y None without relu6) -> gx [B][3][H][W].  Every tap's product [B][OH][OW][3] is added at the
    input pixels (2i-1+kh, 2j-1+kw) of a buffer padded by one pixel."""
    dt = ar.dtype
    B, OH, OW, _ = g.shape
    gz = round_gz(ar, g, scale).to(dt)
    if relu6:
        gz = torch.where(relu6_mask(ar, y.to(dt)), gz, torch.zeros_like(gz))
    wd = w.to(dt)
    acc = torch.zeros(B, H + 2, W + 2, 3, dtype=dt, device=g.device)
    S = torch.zeros_like(acc) if ar.ref else None
    gs = gz.reshape(-1, COUT)
    for kh in range(3):
        for kw in range(3):
            wt = wd[:, :, 2 - kh, 2 - kw] if "flip_taps" in ar.mut else wd[:, :, kh, kw]
            acc[:, kh:kh + 2 * OH - 1:2, kw:kw + 2 * OW - 1:2] += ar.mm(gs, wt).reshape(B, OH, OW, 3)
            if ar.ref:
                S[:, kh:kh + 2 * OH - 1:2, kw:kw + 2 * OW - 1:2] += (gs.abs() @ wt.abs()).reshape(B, OH, OW, 3)
    o = 0 if "parity" in ar.mut else 1                                 # mutant: (h - kh) / 2 instead of (h + 1 - kh) / 2
    crop = lambda a: a[:, o:H + o, o:W + o].permute(0, 3, 1, 2).contiguous()
    istd = _table(ar, inv_std, g).to(dt)
    if "no_inv_std" in ar.mut:
        istd = torch.ones_like(istd)
    return FCOut(crop(acc) * istd + 0.0, None if S is None else crop(S) * istd.abs(), 128, False, out_dtype)


# ---------------------------------------------------------------------------------------------------------- operands
class Operands(NamedTuple):
    x: torch.Tensor              # [B][3][H][W] in the row's stream dtype
    w: torch.Tensor              # [32][3][3][3] bf16
    scale: torch.Tensor          # [32] fp32
    shift: torch.Tensor          # [32] fp32
    g: torch.Tensor              # [B][OH][OW][32] bf16
    mean: tuple
    inv_std: tuple


def operands(name, leg, B, H, W, dtype):
    """leg: 'clamp' / 'rounding' (exact sets) or 'gaussian'.  On the CPU; the GPU tests copy the very same tensors."""
    gen = rng(name, leg)
    OH, OW = out_grid(H, W)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen)
    pick = lambda n: torch.tensor(SCALES)[torch.randint(0, len(SCALES), (n,), generator=gen)]
    if leg == "clamp":
        x, g = ri(-2, 2, B, 3, H, W), ri(-3, 3, B, OH, OW, COUT)
        w = (ri(0, 1, COUT, 3, 3, 3) * 2 - 1) * (torch.rand(COUT, 3, 3, 3, generator=gen) < 1.0 / 9)
        scale = pick(COUT)
        mean, inv_std = EXACT_MEAN, EXACT_INV_STD
        # half-integer shifts that centre the channels n % 3 = 0 / 1 / 2 at -2 / 3 / 8 (mean over the pixels)
        z = first_fwd(Arith(), x.to(dtype), w.to(BF16), mean, inv_std, scale, torch.zeros(COUT), 0).pre
        centre = (z.reshape(-1, COUT).mean(0) * 2).round() / 2
        shift = torch.tensor([-2.0, 3.0, 8.0], dtype=F64)[torch.arange(COUT) % 3] - centre
    elif leg == "rounding":
        x, g = ri(-600, 600, B, 3, H, W), ri(-127, 127, B, OH, OW, COUT)
        w = ri(-15, 15, COUT, 3, 3, 3)
        scale, shift = pick(COUT), ri(-128, 128, COUT) / 2
        mean, inv_std = EXACT_MEAN, EXACT_INV_STD
    else:
        rn = lambda *shape: torch.randn(shape, generator=gen)
        x, g = rn(B, 3, H, W), rn(B, OH, OW, COUT)
        w = rn(COUT, 3, 3, 3) * (3.0 / 27 ** 0.5)
        scale = (0.5 + torch.rand(COUT, generator=gen)) * (ri(0, 1, COUT) * 2 - 1)
        shift = rn(COUT)
        mean, inv_std = IMAGENET_MEAN, tuple(1.0 / s for s in IMAGENET_STD)
    return Operands(x.to(dtype).contiguous(), w.to(BF16).contiguous(), scale.to(F32).contiguous(),
                    shift.to(F32).contiguous(), g.to(BF16).contiguous(), mean, inv_std)


def mask_source(name, leg, y_ref):
    """The y handed to the gradient: the forward's own (reference) output, values 0 and 6 included; in the exact legs half
    of its zeros are turned into -0.0, which the kernel's value comparison must treat as the zero it is."""
    y = y_ref.to(BF16)
    if leg != "gaussian":
        flip = (torch.rand(y.shape, generator=rng(name, leg + "/negzero")) < 0.5) & (y == 0)
        y = torch.where(flip, torch.full_like(y, -0.0), y)
    return y


def pack_fwd(w):
    """[32][3][3][3] -> w_fwd [32][3][4][4] = w[n][c][kh][kw] at [n][kh][kw][c], zero for kw = 3 / c = 3."""
    out = torch.zeros(COUT, 3, 4, 4, dtype=w.dtype, device=w.device)
    out[:, :, :3, :3] = w.permute(0, 2, 3, 1)
    return out.contiguous()


def pack_bwd(w):
    """[32][3][3][3] -> w_bwd [3][9][32] = w[n][c][kh][kw] at [c][kh*3+kw][n], taps NOT flipped."""
    return w.permute(1, 2, 3, 0).reshape(3, 9, COUT).contiguous()


# ---------------------------------------------------------------------------------------------------------- comparators
def assert_premise(name, o):
    """Exact legs, on the reference alone: every value a multiple of the quantum, sum |terms| < 2^24 quanta.  Returns the
    worst sum in quanta and the share of the outputs that are not bf16 values."""
    worst = float(o.S.max()) / QUANTUM
    assert worst < 2.0 ** 24, f"{name}: sum |terms| = {worst:.0f} quanta >= 2^24: the exact leg's premise fails"
    assert bool((o.pre / QUANTUM == (o.pre / QUANTUM).round()).all()), f"{name}: the reference is no multiple of the quantum"
    return worst, float((bf16_rne(o.pre) != o.pre).double().mean())


def branch_shares(v):
    """Shares of v <= 0, 0 < v < 6, v >= 6 (v: a pre-activation, or the stored y of the gradient's mask)."""
    n = v.numel()
    lo, hi = int((v <= 0).sum()), int((v >= 6).sum())
    return lo / n, (n - lo - hi) / n, hi / n


def assert_branches(name, v, least=0.05):
    shares = branch_shares(v)
    assert min(shares) >= least, f"{name}: branch shares {shares}: one of the three ReLU6 branches is nearly empty"
    return shares


def _bits(t, dtype):
    return bits(t) if dtype == BF16 else t.float().contiguous().view(torch.int32)


def compare_exact(name, got, o):
    """got: the kernel's (or emulation's) tensor; o: the reference FCOut.  Raises on any bit that differs (+0 and -0.0
    differ)."""
    want = finish(Arith(), o)
    got = got.reshape(want.shape)
    a, b = _bits(got.cpu(), o.dtype), _bits(want.cpu(), o.dtype)
    if torch.equal(a, b):
        return 0
    bad = (a != b)
    first = tuple(int(v) for v in bad.nonzero()[0])
    raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} outputs differ in bits; first at {first}: "
                         f"got {float(got[first])}, want {float(want[first])} (exact {float(o.pre[first])})")


def gaussian_ratio(got, o):
    """max over elements of |got - r| / bound; bound = 2^-8 |r| + A (1 + 2^-8) for bf16 outputs, A + 2^-24 |r| for fp32."""
    r = expected(o)
    a = acc_eps(o.S, o.n)
    bound = (2.0 ** -8 * (r.abs() + a) + a) if o.dtype == BF16 else (a + 2.0 ** -24 * r.abs())
    return float(((got.reshape(r.shape).double().to(r.device) - r).abs() / bound.clamp_min(2.0 ** -126)).max())


def exact_references(name, leg, B, H, W, dtype):
    """Operands and fp64 references of one exact-leg comparison (clamp: relu6 = 1, rounding: relu6 = 0); every premise is
    asserted on the reference alone.  Returns (op, y for the mask or None, forward reference, gradient reference)."""
    a = 1 if leg == "clamp" else 0
    op = operands(name, leg, B, H, W, dtype)
    ref = first_fwd(Arith(), op.x, op.w, op.mean, op.inv_std, op.scale, op.shift, a)
    worst, inexact = assert_premise(name + "/fwd", ref)
    y = None
    if a:
        y = mask_source(name, leg, finish(Arith(), ref))
        assert_branches(name + "/fwd", ref.pre)
        assert_branches(name + "/mask", y.double())
    else:
        xn = normalise(Arith(mut=("no_round_x",)), op.x, op.mean, op.inv_std)
        x_inexact = float((bf16_rne(xn) != xn).double().mean())
        if op.x.numel() >= 96:                                         # a handful of values may all happen to be bf16 values
            assert x_inexact >= 0.10 and inexact >= 0.10, f"{name}: only {x_inexact:.3f} of x' / {inexact:.3f} of y test the rounding"
    refb = first_bwd(Arith(), op.g, y, op.scale, op.w, op.inv_std, H, W, a, dtype)
    worstb, inexactb = assert_premise(name + "/bwd", refb)
    print(name, "sum |terms| in quanta fwd %.0f bwd %.0f, outputs that need rounding fwd %.2f bwd %.2f" % (worst, worstb, inexact,
                                                                                                         inexactb))
    return op, y, ref, refb


def exact_legs(relu6):
    return (["clamp"] if relu6 else []) + ["rounding"]


def row_name(row, leg):
    B, H, W, dtype, relu6 = row
    return "fc/%s/%s" % ((B, H, W, str(dtype).split(".")[-1], relu6), leg)
