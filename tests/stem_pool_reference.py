"""Restatement of the stem's pooling pair (csrc/adil_stem.hip: adil_maxpool_fwd, adil_stem_pool_bwd), the fp32 emulation
of the backward kernel with its mutants, operand classes and comparators.  Plain torch; works on the CPU and on a GPU.

maxpool_fwd   a selection: nine taps scanned in the order kh*3+kw over whole tensors with a validity mask and a running
              (value, index) pair.  Padding taps do not exist; the first maximum under > wins (+0 == -0: the earlier one
              stays, with its sign); a NaN always replaces the running value, so the last NaN of a window wins.  p carries
              the input's bit pattern; NaN elements are compared as "is NaN".
pool_bwd      the reference in SCATTER form (the kernel gathers): every pooled element with p > 0 by value adds its g, in
              fp64, to the conv-output pixel its idx names.  The kernel forms an fp32 sum of at most four bf16 gradients,
              one fp32 product with scale[c] and one RNE rounding to bf16; the reference forms
              bf16_rne(f32(f32(sum) * scale)), which is the kernel's value bit for bit for ANY fp32 scale whenever the sum
              is exact in fp32 in any order.  That premise is asserted per element on the reference alone: with S = sum
              |terms| and q the smallest bf16 ulp among the non-zero terms, S < 2^24 q (every partial sum is then a multiple
              of q below 2^24 q).  Elements with fewer than two terms satisfy it trivially.  An element off the premise
              (gaussian leg only, capped at 1e-4 of a row) is compared with 2^-8 (|r| + A) + A, A = 4 2^-24 S |scale|; every
              other element bit for bit, zeros as values (no sign of zero is promised for gy).

The operands of a row come from `rng(name, leg)` of classifier_reference on the CPU; GPU tests copy them unchanged."""
from typing import NamedTuple, Optional

import torch

from classifier_reference import (Arith, Out, bf16_rne, bits, Gen, rng, stem_fwd, stem_bwd, operands as classifier_operands,
                                  compare_exact, gaussian_bound, gaussian_ratio, bf16_trunc, BF16, F32, F64)

__all__ = ["Arith", "Out", "bf16_rne", "bits", "Gen", "rng", "stem_fwd", "stem_bwd", "classifier_operands", "compare_exact",
           "gaussian_bound", "gaussian_ratio"]

CANARY = 4096.0                  # exact in bf16; as an idx byte the canary is 0xA5, which is no tap
IDX_CANARY = 0xA5
PREMISE_CAP = 1e-4               # gaussian leg: share of the elements of a row that may be off the exact-sum premise

# (B, OH, OW, C)
SHAPES = [(1, 1, 1, 8), (2, 2, 2, 8), (3, 1, 37, 16), (3, 37, 1, 16), (3, 17, 23, 64), (2, 16, 16, 64), (2, 5, 4, 72),
          (1, 112, 112, 64)]
Y_CLASSES = ("relu", "ints", "negative", "const", "zeros_signed", "special")
EVERY_CLASS_AT = ((3, 17, 23, 64), (2, 16, 16, 64))
PRODUCT_SHAPE = (1, 112, 112, 64)
ZERO_SCALE_ROW = ((2, 5, 4, 72), "relu")         # one channel's scale is 0 here
ZERO_SCALE_CHANNEL = 13
CONST_VALUE = -2.5
NEAR_TIE_SHAPE = (1, 3, 3, 512)     # about 6 % of the channels separate a sum of rounded products from the product of the sum


class Row(NamedTuple):
    shape: tuple
    cls: str                     # a class of Y_CLASSES; "synthetic" (p and idx drawn, no y); "near_tie" (see operands)

    @property
    def name(self):
        return "x".join(str(s) for s in self.shape) + "-" + self.cls


ROWS = ([Row(s, c) for s in SHAPES for c in Y_CLASSES
         if (c == "relu") or (c == "ints" and s != PRODUCT_SHAPE) or (s in EVERY_CLASS_AT)]
        + [Row((3, 17, 23, 64), "synthetic"), Row(NEAR_TIE_SHAPE, "near_tie")])
SMALL_ROWS = [r for r in ROWS if r.shape != PRODUCT_SHAPE]


def pooled(n):
    return (n - 1) // 2 + 1


# ---------------------------------------------------------------------------------------------------------- forward
def _taps(y, origin=-1, bottom_reads_next_image=False):
    """(kh, kw, in-range mask [PH][PW], tap values [B][PH][PW][C]) in scan order."""
    B, OH, OW, C = y.shape
    ph, pw = torch.arange(pooled(OH), device=y.device), torch.arange(pooled(OW), device=y.device)
    nxt = torch.roll(y, -1, 0)
    for kh in range(3):
        oh = 2 * ph + origin + kh
        for kw in range(3):
            ow = 2 * pw + origin + kw
            okh, okw = (oh >= 0) & (oh < OH), (ow >= 0) & (ow < OW)
            v = y[:, oh.clamp(0, OH - 1)][:, :, ow.clamp(0, OW - 1)]
            if bottom_reads_next_image:                                # mutant: row OH of image n is row 0 of image n + 1
                over = oh == OH
                v = torch.where(over[None, :, None, None], nxt[:, torch.zeros_like(oh)][:, :, ow.clamp(0, OW - 1)], v)
                okh = okh | over
            yield kh, kw, okh[:, None] & okw[None, :], v


def maxpool_fwd(y, mut=()):
    """y [B][OH][OW][C], bf16-representable values -> p [B][PH][PW][C] (fp32, the selected element's bits), idx (uint8).
    An fp64 y (an unrounded reference, a bound) is scanned in fp64."""
    y = y if y.dtype == F64 else y.float()
    B, OH, OW, C = y.shape
    shape = (B, pooled(OH), pooled(OW), C)
    zero_start = "start_at_zero" in mut
    best = torch.full(shape, 0.0 if zero_start else float("-inf"), dtype=y.dtype, device=y.device)
    bi = torch.full(shape, 255, dtype=torch.uint8, device=y.device)
    for kh, kw, ok, v in _taps(y, 0 if "origin_2ph" in mut else -1, "next_image" in mut):
        take = (v >= best) if "ge" in mut else (v > best)
        if "nan_loses" not in mut:
            take = take | torch.isnan(v)
        if not zero_start:
            take = take | (bi == 255)                                  # the first tap in range starts the running pair
        take = take & ok[None, :, :, None]
        best = torch.where(take, v, best)
        bi = torch.where(take, torch.full_like(bi, kh + 3 * kw if "idx_transposed" in mut else kh * 3 + kw), bi)
    return best, bi


def tap_pixel(idx, OH, OW):
    """Conv-output pixel (oh, ow), both [B][PH][PW][C] int64, that every idx names, and whether it lies in the grid."""
    B, PH, PW, C = idx.shape
    k = idx.long()
    ph = torch.arange(PH, device=idx.device).view(1, PH, 1, 1)
    pw = torch.arange(PW, device=idx.device).view(1, 1, PW, 1)
    oh, ow = 2 * ph - 1 + k // 3, 2 * pw - 1 + k % 3
    return oh, ow, (k <= 8) & (oh >= 0) & (oh < OH) & (ow >= 0) & (ow < OW)


def same_selection(name, p_got, idx_got, p_want, idx_want, OH, OW):
    """p bit for bit (NaN as NaN), idx byte for byte, every idx a tap in range."""
    p_got, p_want = p_got.float().reshape(p_want.shape), p_want.float()
    nan_g, nan_w = torch.isnan(p_got), torch.isnan(p_want)
    assert torch.equal(nan_g, nan_w), f"{name}: {int((nan_g != nan_w).sum())} elements differ in being NaN"
    a = torch.where(nan_w, torch.zeros_like(p_got), p_got).contiguous().view(torch.int32)
    b = torch.where(nan_w, torch.zeros_like(p_want), p_want).contiguous().view(torch.int32)
    if not torch.equal(a, b):
        bad = (a != b).flatten().nonzero()
        at = int(bad[0])
        raise AssertionError(f"{name}: {bad.numel()} of {a.numel()} pooled values differ in bits; first at flat {at}: got "
                             f"{float(p_got.flatten()[at])}, want {float(p_want.flatten()[at])}")
    idx_got = idx_got.reshape(idx_want.shape)
    if not torch.equal(idx_got, idx_want):
        bad = (idx_got != idx_want).flatten().nonzero()
        at = int(bad[0])
        raise AssertionError(f"{name}: {bad.numel()} of {idx_want.numel()} idx bytes differ; first at flat {at}: got "
                             f"{int(idx_got.flatten()[at])}, want {int(idx_want.flatten()[at])}")
    assert bool(tap_pixel(idx_got, OH, OW)[2].all()), f"{name}: an idx names no tap in range"


# --------------------------------------------------------------------------------------------------------- backward
class GyRef(NamedTuple):
    sum: torch.Tensor            # fp64 [B][OH][OW][C]: the routed, masked gradients, added
    S: torch.Tensor              # sum |terms|
    n: torch.Tensor              # number of non-zero terms
    q: torch.Tensor              # smallest bf16 ulp among the non-zero terms (inf where there is none)
    scale: torch.Tensor          # fp32 [C] (fp64 as handed in: an unrounded reference)

    @property
    def want(self):
        """bf16_rne(f32(f32(sum) * scale)) as fp32 values."""
        return gy_of(Arith(), self)

    @property
    def exact_sum(self):
        """Per element: the fp32 sum is exact in any order."""
        return (self.n < 2) | (self.S < 2.0 ** 24 * self.q)

    @property
    def bound(self):
        """For an element off the premise: 2^-8 (|r| + A) + A, A = 4 2^-24 S |scale|."""
        sc = self.scale.double().abs()
        A = 4 * 2.0 ** -24 * self.S * sc
        return 2.0 ** -8 * ((self.sum * self.scale.double()).abs() + A) + A


def gy_of(ar, ref):
    """gy of a GyRef in the arithmetic `ar`: rnd(f32(f32(sum) * scale)); over `Unrounded` the real product."""
    return ar.rnd(ar.f32(ar.f32(ref.sum) * ar.f32(ref.scale)))


def bf16_ulp(v):
    """ulp of the bf16 binade of |v| (v != 0, normal)."""
    _, e = torch.frexp(v.double().abs())
    return torch.ldexp(torch.ones_like(v, dtype=F64), e - 8)


def pool_bwd(g, idx, p, scale, OH, OW):
    """Scatter form, fp64.  g, idx, p [B][PH][PW][C]; scale [C] fp32.  Every idx must name a tap in range."""
    B, PH, PW, C = g.shape
    dev = g.device
    oh, ow, ok = tap_pixel(idx, OH, OW)
    assert bool(ok.all()), "pool_bwd: an idx names no tap in range"
    keep = p.float() > 0                                               # by value: -0, negatives and NaN fail
    b = torch.arange(B, device=dev).view(B, 1, 1, 1)
    c = torch.arange(C, device=dev).view(1, 1, 1, C)
    flat = (((b * OH + oh) * OW + ow) * C + c)[keep]
    t = g.double()[keep]
    n_el = B * OH * OW * C
    z = lambda: torch.zeros(n_el, dtype=F64, device=dev)
    s = z().index_add_(0, flat, t)
    S = z().index_add_(0, flat, t.abs())
    nz = t != 0
    n = z().index_add_(0, flat[nz], torch.ones_like(t[nz]))
    q = torch.full((n_el,), float("inf"), dtype=F64, device=dev)
    q = q.scatter_reduce(0, flat[nz], bf16_ulp(t[nz]), "amin")
    shape = (B, OH, OW, C)
    return GyRef(s.view(shape), S.view(shape), n.view(shape), q.view(shape), scale if scale.dtype == F64 else scale.float())


MUTANTS_FWD = ("ge", "start_at_zero", "nan_loses", "idx_transposed", "origin_2ph", "next_image")
MUTANTS_BWD = ("mask_ge", "no_mask", "first_window_only", "clamped_window", "neighbour_scale", "trunc", "scale_each_term")


def emulate_pool_bwd(g, idx, p, scale, OH, OW, mut=()):
    """The kernel's gather form in fp32: every conv-output pixel visits the at most 2 x 2 windows that contain it, in
    ascending (ph, pw) order."""
    B, PH, PW, C = g.shape
    dev = g.device
    gf, pf, k = g.float(), p.float(), idx.long()
    sc = scale.float()
    if "neighbour_scale" in mut:
        sc = torch.roll(sc, 1)
    oh, ow = torch.arange(OH, device=dev), torch.arange(OW, device=dev)
    acc = torch.zeros(B, OH, OW, C, dtype=F32, device=dev)
    if "mask_ge" in mut:
        pos = pf >= 0
    elif "no_mask" in mut:
        pos = torch.ones_like(pf, dtype=torch.bool)
    else:
        pos = pf > 0
    for a in range(2):
        ph = oh // 2 + a
        on_h = a < 1 + (oh & 1)
        if "clamped_window" in mut:
            ph = ph.clamp_max(PH - 1)
        else:
            on_h = on_h & (ph < PH)
        kh = oh - (2 * ph.clamp_max(PH - 1) - 1)
        for b in range(2):
            if "first_window_only" in mut and (a or b):
                continue
            pw = ow // 2 + b
            on_w = b < 1 + (ow & 1)
            if "clamped_window" in mut:
                pw = pw.clamp_max(PW - 1)
            else:
                on_w = on_w & (pw < PW)
            kw = ow - (2 * pw.clamp_max(PW - 1) - 1)
            want = (kh[:, None] * 3 + kw[None, :])[None, :, :, None]
            on = (on_h[:, None] & on_w[None, :])[None, :, :, None]
            sel = lambda t: t[:, ph.clamp_max(PH - 1)][:, :, pw.clamp_max(PW - 1)]
            hit = on & (sel(k) == want) & sel(pos)
            term = torch.where(hit, sel(gf), torch.zeros((), dtype=F32, device=dev))
            if "scale_each_term" in mut:
                term = term * sc
            acc = acc + term
    if "scale_each_term" not in mut:
        acc = acc * sc
    return bf16_trunc(acc) if "trunc" in mut else bf16_rne(acc)


class GyReport(NamedTuple):
    off_premise: int             # elements compared with the bound
    elements: int
    worst_ratio: float           # max |got - r| / bound over them (0 when there is none)


def compare_gy(name, got, ref, exact_leg):
    """Every element on the premise bit for bit (zeros as values), the others within their bound; the exact leg has none."""
    want = ref.want
    got = got.float().reshape(want.shape)
    on = ref.exact_sum
    off = int((~on).sum())
    if exact_leg:
        assert off == 0, f"{name}: {off} elements off the exact-sum premise on the exact leg"
    assert off <= PREMISE_CAP * on.numel(), f"{name}: {off} of {on.numel()} elements off the exact-sum premise: above the cap"
    a, b = bits(got + 0.0), bits(want + 0.0)                           # -0 + 0 = +0: zeros compare as values
    bad = (a != b) & on
    if bool(bad.any()):
        at = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} gy elements differ in bits; first at flat {at}: got "
                             f"{float(got.flatten()[at])}, want {float(want.flatten()[at])} (sum {float(ref.sum.flatten()[at])})")
    worst = 0.0
    if off:
        r = ref.sum * ref.scale.double()
        ratio = ((got.double() - r).abs() / ref.bound.clamp_min(2.0 ** -126))[~on]
        worst = float(ratio.max())
        assert worst <= 1.0, f"{name}: an element off the premise is {worst:.3f} of its bound"
    return GyReport(off, on.numel(), worst)


def rounding_stats(ref):
    """(share non-zero, share really rounded, share exact ties) of the final rounding of an exact-leg gy."""
    pre = ref.sum.float() * ref.scale.float()
    lo = bf16_trunc(pre)
    rounded = lo != pre
    ulp = bf16_ulp(torch.where(lo == 0, torch.ones_like(lo), lo)).float()
    tie = rounded & ((pre - lo).abs() * 2 == ulp)
    return float((pre != 0).double().mean()), float(rounded.double().mean()), float(tie.double().mean())


# --------------------------------------------------------------------------------------------------------- operands
def _y(row, g):
    shape, cls = row.shape, row.cls
    if cls == "relu":
        return torch.relu(torch.randn(shape, generator=g)).to(BF16)
    if cls == "ints":
        return torch.randint(-3, 4, shape, generator=g).to(BF16)
    if cls == "negative":
        return (-torch.randn(shape, generator=g).abs() - 1).to(BF16)
    if cls == "const":
        return torch.full(shape, CONST_VALUE).to(BF16)
    if cls == "zeros_signed":
        return torch.where(torch.rand(shape, generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0)).to(BF16)
    if cls == "special":
        y = torch.randn(shape, generator=g)
        u = torch.rand(shape, generator=g)
        y = torch.where(u < 0.01, torch.tensor(float("inf")), y)
        y = torch.where((u >= 0.01) & (u < 0.02), torch.tensor(float("-inf")), y)
        y = torch.where((u >= 0.02) & (u < 0.03), torch.tensor(float("nan")), y)
        y[0, 0:2, 0:2, 0] = float("-inf")                              # the corner window (0, 0) of channel 0: only -inf
        y[0, 3:6, 3:6, 1] = 0.5                                        # window (2, 2) of channel 1: two NaNs, taps 1 and 5
        y[0, 3, 4, 1] = y[0, 4, 5, 1] = float("nan")
        return y.to(BF16)
    raise KeyError(cls)


def special_windows(y):
    """(windows with at least two NaNs, windows whose every tap in range is -inf) of a `special` y."""
    nans = torch.zeros(y.shape[0], pooled(y.shape[1]), pooled(y.shape[2]), y.shape[3])
    all_ninf = torch.ones_like(nans, dtype=torch.bool)
    for _, _, ok, v in _taps(y.float()):
        m = ok[None, :, :, None]
        nans += (torch.isnan(v) & m).float()
        all_ninf &= (v == float("-inf")) | ~m
    return int((nans >= 2).sum()), int(all_ninf.sum())


def _g_scale(name, leg, pshape):
    G = Gen(name + "/g", leg)
    C = pshape[-1]
    if leg == "exact":
        g = torch.randint(-255, 256, pshape, generator=G.g).to(BF16)
        scale = G.scale(C) * torch.where(torch.arange(C) % 2 == 0, 1.5, 1.0)
    else:
        g = torch.randn(pshape, generator=G.g).to(BF16)
        scale = G.scale(C)
    return g, scale.float().contiguous()


def operands(row, leg):
    """CPU tensors of a row.  Classes of Y_CLASSES: y (bf16), g (bf16), scale (fp32).  `synthetic`: p drawn from
    {-1, -0.0, +0.0, 1, NaN} independently of idx, idx a random tap in range, no y.  `near_tie`: one 3 x 3 image whose
    centre pixel is named by all four windows; g are integers in [128, 255] and scale[c] is the fp32 nearest T / sum(g) for
    a bf16 tie T, so f32(sum * scale) sits on the tie while a sum of separately rounded products leaves it."""
    B, OH, OW, C = row.shape
    pshape = (B, pooled(OH), pooled(OW), C)
    gen = rng(row.name, leg)
    if row.cls == "near_tie":
        assert (OH, OW) == (3, 3)
        g = torch.randint(128, 256, pshape, generator=gen)
        tie = 257.0 + 2 * torch.randint(0, 64, (C,), generator=gen)     # odd integers in [257, 383]: ties of the binade [256, 512)
        assert B == 1
        scale = (tie.double() / g.sum((0, 1, 2)).double()).float()
        scale = scale * (torch.randint(0, 2, (C,), generator=gen).float() * 2 - 1)
        kh = 2 - 2 * torch.arange(2).view(1, 2, 1, 1)                   # window (ph, pw): pixel (1, 1) is tap (2 - 2ph, 2 - 2pw)
        kw = 2 - 2 * torch.arange(2).view(1, 1, 2, 1)
        idx = (kh * 3 + kw).expand(pshape).to(torch.uint8).contiguous()
        return dict(p=torch.ones(pshape, dtype=BF16), idx=idx, g=g.to(BF16), scale=scale.contiguous())
    g, scale = _g_scale(row.name, leg, pshape)
    if row.cls == "synthetic":
        vals = torch.tensor([-1.0, -0.0, 0.0, 1.0, float("nan")])
        p = vals[torch.randint(0, 5, pshape, generator=gen)].to(BF16)
        k = torch.randint(0, 9, pshape, generator=gen).to(torch.uint8)
        idx = torch.where(tap_pixel(k, OH, OW)[2], k, torch.full_like(k, 4))   # the centre tap is always in range
        return dict(p=p, idx=idx, g=g, scale=scale)
    if (row.shape, row.cls) == ZERO_SCALE_ROW:
        scale[ZERO_SCALE_CHANNEL] = 0.0
    return dict(y=_y(row, gen), g=g, scale=scale)


def forward_of(row, o):
    """(p, idx) a row's backward takes: the restatement of its y, or the drawn pair."""
    if "y" in o:
        return maxpool_fwd(o["y"])
    return o["p"].float(), o["idx"]
