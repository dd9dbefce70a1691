"""float64 restatement of the VGG first-group kernels (csrc/adil_vgg_first.hip: adil_first3x3_pool_fwd / _bwd), their
operand generators and comparators, written over `classifier_reference.Arith` in the manner of
tests/first_conv_reference.py (whose `normalise` forms x' here too).  The pool rule is `vgg_conv_reference.pool_restate`,
by import.  Plain torch, on the CPU.

    forward    x' = bf16(f32(f32(x - mean[c]) * inv_std[c])), zero padded AFTER the normalisation;
               s[b][h][w][n] = sum x'[b][c][h-1+kh][w-1+kw] w[n][c][kh][kw];  t = s + bias[n] (one fp32 add);
               per 2x2 window the first of (0,0), (0,1), (1,0), (1,1) strictly greater than all before it wins, on t;
               y = bf16(max(t_winner, 0)) with zeros +0;  idx = 2 dh + dw, or 4 where t_winner <= 0
    gradient   gz[h][w][n] = bits of g[h/2][w/2][n] where idx == 2 (h & 1) + (w & 1), else +0;
               gx[b][c][h][w] = round(inv_std[c] * sum gz[b][h+1-kh][w+1-kw][n] w[n][c][kh][kw])

x and gx are [B][3][H][W] (fp32 or bf16), y, idx and g [B][H/2][W/2][64], w [64][3][3][3] bf16, bias [64] fp32.

exact legs    everything on the quantum grid of first_conv_reference (1/4): integer x, mean (1, 0, -1), inv_std (1, 1/2, 2),
              integer w, bias on the half-integer grid, integer g.  Every product, every partial sum in ANY order and t are
              multiples of the quantum below 2^24 quanta, exact in fp32, so the one correct result is the rounding of the
              exact value and y, idx and gx are compared BIT FOR BIT, the sign of zeros included.  Premises are asserted on
              the reference alone.
                tie set       x in [-1, 1], w = +-1 with density 1/9, g in [-3, 3]; per channel the bias puts the 8 %
                              quantile of the window maxima at zero, so tied maxima and dead windows are both common
                              (asserted: in every row of >= 100 windows >= 10 % live windows with a tied maximum, >= 5 %
                              dead windows, and every idx value 0..4 occurs).
                rounding set  |x| <= 600, |w| <= 15, |g| <= 127: x', y and gx need more than 8 bits (asserted: >= 10 % of x'
                              and of t_winner are not bf16 values, in rows of >= 100 values).
gaussian leg  N(0,1) x, w, g and bias, the ImageNet mean and std.  The operands of both sums are the same bits on both
              sides, so the only errors are those of the fp32 accumulation and of the last rounding:
              A = acc_eps(S, n) as derived in first_conv_reference, n = 28 forward (27 products and the bias), n = 576
              backward (9 taps of 64 channels; the product with inv_std is the epilogue operation the factor 2 covers).
                y      r = max(0, max_window t_ref).  The kernel's y is max(0, t_k[k']) for its own winner k', every
                       |t_k[k] - t_ref[k]| <= A[k], and the maximum is 1-Lipschitz in the sup norm, so with
                       A = max_window A[k]:  |y - r| <= 2^-8 |r| + A (1 + 2^-8).
                idx    a window is DECIDED when the top two t_ref differ by more than 2 A and |max t_ref| > A; there idx
                       must equal the reference's.  On an undecided window the kernel's choice k must satisfy
                       t_ref[k] >= max t_ref - 2 A, or be 4 with max t_ref <= A.  No window is excluded; undecided windows
                       may be at most 0.1 % of a row (asserted on the reference alone).
                gx     fed the REFERENCE's idx, so both sides sum the same bits; bound as in first_conv_reference.

Every operation is written once over an `Arith`: fp64 is the reference; fp32 with one partial sum per MFMA (a tap row
forward; half a tap's channels backward, in the kernel's order) is the CPU emulation of the kernel, which also takes the
mutants of tests/test_vgg_first_cpu.py."""
import functools
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from classifier_reference import BF16, F32, F64, Arith, acc_eps, bf16_rne, bits, rng
from first_conv_reference import EXACT_INV_STD, EXACT_MEAN, IMAGENET_MEAN, IMAGENET_STD, QUANTUM, _table, normalise
from vgg_conv_reference import PoolOperands, pool_restate, same_bits  # noqa: F401

COUT = 64
FWD_TILE = (16, 32)              # input pixels (H, W) of a first3x3_pool_fwd workgroup
BWD_TILE = (16, 32)              # input pixels (H, W) of a first3x3_pool_bwd workgroup
CORNERS = ((0, 0), (0, 1), (1, 0), (1, 1))


def _tile_shapes(tile):
    th, tw = tile
    return [(1, h, w) for h in (th - 2, th, th + 2) for w in (tw - 2, tw, tw + 2)]


# (B, H, W): the five small shapes; H in {TH-2, TH, TH+2} x W in {TW-2, TW, TW+2} around each kernel's tile (the two tiles
# are the same size as built, so the nine shapes serve both); two images across a tile edge; one image at 224 x 224
SHAPES = [(1, 2, 2), (3, 6, 10), (2, 8, 8), (1, 2, 34), (1, 34, 2)]
for _s in _tile_shapes(FWD_TILE) + _tile_shapes(BWD_TILE):
    if _s not in SHAPES:
        SHAPES.append(_s)
# (B, H, W, x dtype): both stream dtypes, alternating; two images across a tile edge in both, the 224 x 224 image in bf16
ROWS = ([s + ((BF16, F32)[i % 2],) for i, s in enumerate(SHAPES)]
        + [(2, 18, 34, BF16), (2, 18, 34, F32), (1, 224, 224, BF16)])
OOB_ROWS = [(1, 6, 10), (1, FWD_TILE[0] + 2, FWD_TILE[1] + 2)]
HASH_ROWS = [(3, 6, 10, F32), (2, 18, 34, BF16), (1, 14, 30, F32)]
EXACT_LEGS = ("tie", "rounding")


def row_name(row, leg):
    B, H, W, dtype = row
    return "vf/%s/%s" % ((B, H, W, str(dtype).split(".")[-1]), leg)


# ------------------------------------------------------------------------------------------------------------- forward
class Pre(NamedTuple):
    s: torch.Tensor                        # [B][H][W][64] the convolution sum, in the arithmetic's dtype
    S: Optional[torch.Tensor]              # sum |terms| of s (reference only)


def conv_sum(ar, x, w, mean, inv_std):
    """s [B][H][W][64]; one partial sum per tap row, K order (kw, c): the kernel's MFMA step."""
    dt = ar.dtype
    B, _, H, W = x.shape
    if "raw_pad" in ar.mut:                                            # mutant: the padding is applied in raw-pixel space
        xp = normalise(ar, F.pad(x.float(), (1, 1, 1, 1)), mean, inv_std).to(dt)
    else:
        xp = F.pad(normalise(ar, x, mean, inv_std).to(dt), (1, 1, 1, 1))
    wd = w.to(dt)
    if "chan_order" in ar.mut:                                         # mutant: the input channels are read in reverse order
        wd = wd.flip(1)
    acc = torch.zeros(B * H * W, COUT, dtype=dt)
    S = torch.zeros_like(acc) if ar.ref else None
    for kh in range(3):
        cols = torch.cat([xp[:, :, kh:kh + H, kw:kw + W].permute(0, 2, 3, 1).reshape(-1, 3) for kw in range(3)], 1)
        wk = wd[:, :, kh].permute(0, 2, 1).reshape(COUT, 9)
        acc = acc + ar.mm(cols, wk.t())
        if ar.ref:
            S += cols.abs() @ wk.abs().t()
    shape = (B, H, W, COUT)
    return Pre(acc.reshape(shape) + 0.0, None if S is None else S.reshape(shape))


class FwdOut(NamedTuple):
    y: torch.Tensor                        # [B][H/2][W/2][64] bf16
    idx: torch.Tensor                      # [B][H/2][W/2][64] uint8
    t: torch.Tensor                        # [B][H][W][64] s + bias in the arithmetic's dtype
    S: Optional[torch.Tensor]              # sum |terms| of t


def first_pool_fwd(ar, x, w, bias, mean, inv_std):
    """The forward on the exact legs and in the emulation: `pool_restate` decides on fp32(s) + bias, which IS the kernel's
    operation sequence in the emulation and is exact for the reference on the exact legs (asserted by `assert_premise`)."""
    pre = conv_sum(ar, x, w, mean, inv_std)
    mut = tuple(m for m in ("last_winner", "dead_passes", "bias_after_max") if m in ar.mut)
    out = pool_restate(PoolOperands(pre.s, bias.float(), torch.zeros(pre.s[:, ::2, ::2].shape, dtype=BF16)), mut)
    y = out.y
    if "neg_zero" in ar.mut:                                           # mutant: -0.0 is emitted
        y = torch.where(y == 0, torch.full_like(y, -0.0), y)
    t = pre.s + bias.to(ar.dtype)
    return FwdOut(y, out.idx, t, None if pre.S is None else pre.S + bias.to(ar.dtype).abs())


def windows(t):
    """[B][H][W][C] -> [4][B][H/2][W/2][C], corner k = 2 dh + dw."""
    return torch.stack([t[:, dh::2, dw::2] for dh, dw in CORNERS])


# ------------------------------------------------------------------------------------------------------------ gradient
class BwdOut(NamedTuple):
    pre: torch.Tensor                      # [B][3][H][W] before the rounding
    S: Optional[torch.Tensor]
    n: int
    dtype: torch.dtype


def unpool(ar, g, idx):
    """gz [B][H][W][64] bf16: the bits of g at the winner, +0 elsewhere."""
    B, OH, OW, C = g.shape
    gz = torch.zeros((B, 2 * OH, 2 * OW, C), dtype=BF16)
    sel = (idx & 3) if "dead_passes_bwd" in ar.mut else idx            # mutant: a dead window passes its gradient to (0, 0)
    for k, (dh, dw) in enumerate(CORNERS):
        gz[:, dh::2, dw::2] = torch.where(sel == k, g, torch.zeros((), dtype=BF16))
    return gz


def first_pool_bwd(ar, g, idx, w, inv_std, out_dtype=BF16):
    """g [B][H/2][W/2][64] bf16, idx uint8 -> gx [B][3][H][W].  Per accumulator the taps in the order kh * 3 + kw, within a
    tap channels 0..31 (one MFMA) before 32..63 (the next)."""
    dt = ar.dtype
    gz = unpool(ar, g, idx)
    B, H, W, _ = gz.shape
    gzp = F.pad(gz.to(dt), (0, 0, 1, 1, 1, 1))
    wd = w.to(dt)
    acc = torch.zeros(B * H * W, 3, dtype=dt)
    S = torch.zeros_like(acc) if ar.ref else None
    for kh in range(3):
        for kw in range(3):
            wt = wd[:, :, 2 - kh, 2 - kw] if "flip_taps" in ar.mut else wd[:, :, kh, kw]
            src = gzp[:, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W].reshape(-1, COUT)
            for half in (slice(0, 32), slice(32, 64)):
                acc = acc + src[:, half] @ wt[half]
            if ar.ref:
                S += src.abs() @ wt.abs()
    istd = _table(ar, inv_std, g).to(dt)
    to_nchw = lambda a: a.reshape(B, H, W, 3).permute(0, 3, 1, 2).contiguous()
    return BwdOut(to_nchw(acc) * istd + 0.0, None if S is None else to_nchw(S) * istd.abs(), 576, out_dtype)


def finish_bwd(ar, o):
    v = o.pre + 0.0
    return ar.rnd(v) if o.dtype == BF16 else ar.f32(v).to(v.dtype)


# ---------------------------------------------------------------------------------------------------------- operands
class Operands(NamedTuple):
    x: torch.Tensor              # [B][3][H][W] in the row's stream dtype
    w: torch.Tensor              # [64][3][3][3] bf16
    bias: torch.Tensor           # [64] fp32
    g: torch.Tensor              # [B][H/2][W/2][64] bf16
    mean: tuple
    inv_std: tuple


def operands(name, leg, B, H, W, dtype):
    """leg: 'tie' / 'rounding' (exact sets) or 'gaussian'."""
    gen = rng(name, leg)
    OH, OW = H // 2, W // 2
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen)
    if leg == "tie":
        x, g = ri(-1, 1, B, 3, H, W), ri(-3, 3, B, OH, OW, COUT)
        w = (ri(0, 1, COUT, 3, 3, 3) * 2 - 1) * (torch.rand(COUT, 3, 3, 3, generator=gen) < 1.0 / 9)
        mean, inv_std = EXACT_MEAN, EXACT_INV_STD
        s = conv_sum(Arith(), x.to(dtype), w.to(BF16), mean, inv_std).s
        top = windows(s).max(0).values.reshape(-1, COUT)
        bias = -(top.quantile(0.08, 0, interpolation="lower") * 2).round() / 2     # half-integer grid
    elif leg == "rounding":
        x, g = ri(-600, 600, B, 3, H, W), ri(-127, 127, B, OH, OW, COUT)
        w = ri(-15, 15, COUT, 3, 3, 3)
        bias = ri(-128, 128, COUT) / 2
        mean, inv_std = EXACT_MEAN, EXACT_INV_STD
    else:
        rn = lambda *shape: torch.randn(shape, generator=gen)
        x, g, w, bias = rn(B, 3, H, W), rn(B, OH, OW, COUT), rn(COUT, 3, 3, 3), rn(COUT)
        mean, inv_std = IMAGENET_MEAN, tuple(1.0 / s for s in IMAGENET_STD)
    return Operands(x.to(dtype).contiguous(), w.to(BF16).contiguous(), bias.to(F32).contiguous(), g.to(BF16).contiguous(),
                    mean, inv_std)


def pack_fwd(w):
    """[64][3][3][3] -> w_fwd [64][3][4][4] = w[n][c][kh][kw] at [n][kh][kw][c], zero for kw = 3 / c = 3."""
    out = torch.zeros(COUT, 3, 4, 4, dtype=w.dtype, device=w.device)
    out[:, :, :3, :3] = w.permute(0, 2, 3, 1)
    return out.contiguous()


def pack_bwd(w):
    """[64][3][3][3] -> w_bwd [3][9][64] = w[n][c][kh][kw] at [c][kh*3+kw][n], taps NOT flipped."""
    return w.permute(1, 2, 3, 0).reshape(3, 9, COUT).contiguous()


# ---------------------------------------------------------------------------------------------------------- comparators
def _quanta(name, v, S):
    worst = float(S.max()) / QUANTUM
    assert worst < 2.0 ** 24, f"{name}: sum |terms| = {worst:.0f} quanta >= 2^24: the exact leg's premise fails"
    assert bool((v / QUANTUM == (v / QUANTUM).round()).all()), f"{name}: the reference is no multiple of the quantum"
    return worst


class ExactRow(NamedTuple):
    op: Operands
    fwd: FwdOut
    bwd: BwdOut
    shares: dict


@functools.lru_cache(maxsize=None)
def exact_references(row, leg):
    """Operands and fp64 references of one exact-leg row, computed once and shared, never modified; every premise is
    asserted here, on the reference alone."""
    B, H, W, dtype = row
    name = row_name(row, leg)
    op = operands(name, leg, B, H, W, dtype)
    ref = first_pool_fwd(Arith(), op.x, op.w, op.bias, op.mean, op.inv_std)
    _quanta(name + "/fwd", ref.t, ref.S)
    win = windows(ref.t)
    top = win.max(0).values
    n = top.numel()
    shares = dict(tied=float((((win == top).sum(0) > 1) & (top > 0)).double().mean()), dead=float((top <= 0).double().mean()),
                  idx=sorted(set(ref.idx.reshape(-1).tolist())))
    if leg == "tie" and n >= 100:
        assert shares["tied"] >= 0.10 and shares["dead"] >= 0.05, f"{name}: live tied {shares['tied']:.3f}, dead {shares['dead']:.3f}"
        assert shares["idx"] == [0, 1, 2, 3, 4], f"{name}: idx values {shares['idx']}"
    if leg == "rounding":
        xn = normalise(Arith(mut=("no_round_x",)), op.x, op.mean, op.inv_std)
        shares["x_inexact"] = float((bf16_rne(xn) != xn).double().mean())
        shares["y_inexact"] = float((bf16_rne(top) != top).double().mean())
        if n >= 100 and op.x.numel() >= 100:
            assert shares["x_inexact"] >= 0.10 and shares["y_inexact"] >= 0.10, f"{name}: {shares}"
    refb = first_pool_bwd(Arith(), op.g, ref.idx, op.w, op.inv_std, dtype)
    _quanta(name + "/bwd", refb.pre, refb.S)
    return ExactRow(op, ref, refb, shares)


def _differ(name, a, b, got, want):
    if torch.equal(a, b):
        return
    bad = a != b
    first = tuple(int(v) for v in bad.nonzero()[0])
    raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} outputs differ in bits; first at {first}: "
                         f"got {float(got[first])}, want {float(want[first])}")


def compare_fwd_exact(name, y, idx, ref):
    """Raises on any bit of y (+0 and -0.0 differ) or any idx byte that differs."""
    y, idx = y.cpu().reshape(ref.y.shape), idx.cpu().reshape(ref.idx.shape)
    _differ(name + "/idx", idx, ref.idx, idx, ref.idx)
    _differ(name + "/y", bits(y), bits(ref.y), y, ref.y)


def compare_bwd_exact(name, gx, refb):
    want = finish_bwd(Arith(), refb)
    gx = gx.cpu().reshape(want.shape)
    view = (lambda t: bits(t)) if refb.dtype == BF16 else (lambda t: t.float().contiguous().view(torch.int32))
    _differ(name + "/gx", view(gx), view(want), gx, want)


class GaussRow(NamedTuple):
    op: Operands
    win: torch.Tensor            # [4][B][OH][OW][64] t_ref per corner
    A: torch.Tensor              # [B][OH][OW][64] max over the window of acc_eps(S, 28)
    idx: torch.Tensor            # the reference's idx
    decided: torch.Tensor        # bool
    bwd: BwdOut                  # from the reference's idx


@functools.lru_cache(maxsize=None)
def gaussian_references(row):
    B, H, W, dtype = row
    name = row_name(row, "gaussian")
    op = operands(name, "gaussian", B, H, W, dtype)
    ar = Arith()
    pre = conv_sum(ar, op.x, op.w, op.mean, op.inv_std)
    t, S = pre.s + op.bias.double(), pre.S + op.bias.double().abs()
    win, A = windows(t), acc_eps(windows(S), 28).max(0).values
    top, arg = win.max(0)
    first = (win == top).double().argmax(0)                            # the first corner that holds the maximum
    idx = torch.where(top <= 0, torch.full_like(first, 4), first).to(torch.uint8)
    second = win.scatter(0, arg[None], float("-inf")).max(0).values
    decided = ((top - second) > 2 * A) & (top.abs() > A)
    share = 1.0 - float(decided.double().mean())
    assert share <= 1e-3, f"{name}: {share:.5f} of the windows are undecided"
    return GaussRow(op, win, A, idx, decided, first_pool_bwd(ar, op.g, idx, op.w, op.inv_std, dtype))


def gaussian_fwd(name, y, idx, ref):
    """(max |y - r| / bound, number of undecided windows); raises where idx breaks its rule."""
    y, idx = y.cpu().reshape(ref.A.shape).double(), idx.cpu().reshape(ref.A.shape)
    top = ref.win.max(0).values
    r = top.clamp_min(0.0)
    ratio = float(((y - r).abs() / (2.0 ** -8 * (r.abs() + ref.A) + ref.A).clamp_min(2.0 ** -126)).max())
    wrong = ref.decided & (idx != ref.idx)
    assert not bool(wrong.any()), f"{name}: idx differs on {int(wrong.sum())} decided windows"
    assert bool((idx <= 4).all()), f"{name}: idx above 4"
    chosen = ref.win.gather(0, idx.clamp_max(3).long()[None])[0]
    ok = torch.where(idx == 4, top <= ref.A, chosen >= top - 2 * ref.A)
    bad = ~ref.decided & ~ok
    assert not bool(bad.any()), f"{name}: idx outside its allowance on {int(bad.sum())} undecided windows"
    return ratio, int((~ref.decided).sum())


def gaussian_bwd_ratio(gx, o):
    r = o.pre
    a = acc_eps(o.S, o.n)
    bound = (2.0 ** -8 * (r.abs() + a) + a) if o.dtype == BF16 else (a + 2.0 ** -24 * r.abs())
    return float(((gx.cpu().reshape(r.shape).double() - r).abs() / bound.clamp_min(2.0 ** -126)).max())
