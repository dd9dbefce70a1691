"""float64 restatement of the depthwise 3x3 kernels (csrc/adil_depthwise.hip: adil_dw3x3_fwd / adil_dw3x3_bwd), their
operand generators and comparators, written over `classifier_reference.Arith`.  Plain torch; CPU or GPU.

The kernels multiply bf16 activations with fp32 weights, accumulate in fp32 and round ONCE to bf16, to nearest even;
ReLU6 clamps the fp32 value before the rounding (0 and 6 are bf16 values and rounding is monotone, so clamping after the
rounding gives the same bits).  As in classifier_reference there are two legs:

exact leg     integer operands whose every partial sum is an integer below 2^23: exact in fp32 in ANY order, so the one
              correct output is the RNE bf16 rounding of the exact value and a kernel is compared BIT FOR BIT.
                clamp set     x in [-3,3], w in [-2,2], bias in [-3,6], g in [-3,3]: every value is a bf16 value, and the
                              three ReLU6 branches pre <= 0, 0 < pre < 6, pre >= 6 are all well populated (asserted);
                rounding set  relu6 = 0, |x| <= 127, |w| <= 15: outputs need more than 8 bits, so RNE itself is tested
                              (asserted: at least 10 % of the reference outputs are not bf16 values).
gaussian leg  N(0,1) operands; elementwise bound, derived, not measured:
                  |out - r| <= 2^-8 |r| + A (1 + 2^-8),   A = n 2^-24 S 2,  n = 10 (9 taps + bias)
              r = expected output in fp64 after the clamp (forward; the clamp is 1-Lipschitz) / with the mask applied
              (gradient; the mask comes from the y handed in, so it is the same on both sides), S = sum |terms|.
              No element is excluded.

Every operation is written once over an `Arith`: fp64 is the reference; fp32, accumulated tap by tap in the kernel's order
(kh*3+kw ascending, then the bias), is the CPU emulation of the kernel, which also takes the mutants of
tests/test_depthwise_cpu.py."""
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from classifier_reference import BF16, CANARY, F32, F64, Arith, acc_eps, bf16_rne, bits, rng

N_TERMS = 10                     # 9 taps + bias

# (C, H, stride) of the 17 depthwise layers of MobileNetV2 at 224 x 224 in network order (H = W = input grid of the layer;
# tests/test_depthwise_cpu.py derives the list from the network itself) and the distinct ones among them: 10 shapes
MOBILENET_SHAPES = [(32, 112, 1), (96, 112, 2), (144, 56, 1), (144, 56, 2), (192, 28, 1), (192, 28, 2), (384, 14, 1),
                    (576, 14, 1), (576, 14, 2), (960, 7, 1)]
MOBILENET_SHAPES_ALL17 = [(32, 112, 1), (96, 112, 2), (144, 56, 1), (144, 56, 2), (192, 28, 1), (192, 28, 1), (192, 28, 2),
                          (384, 14, 1), (384, 14, 1), (384, 14, 1), (384, 14, 1), (576, 14, 1), (576, 14, 1), (576, 14, 2),
                          (960, 7, 1), (960, 7, 1), (960, 7, 1)]
# (channels, stride) of the 17 layers in network order: what `own_depthwise=True` must replace
MOBILENET_LAYERS = [(c, s) for c, _, s in MOBILENET_SHAPES_ALL17]


def out_size(n, stride):
    return (n - 1) // stride + 1


class DwOut(NamedTuple):
    pre: torch.Tensor                      # the value before the clamp and the rounding
    S: Optional[torch.Tensor]              # sum |terms| of pre (reference only)
    relu6: bool = False                    # clamp to [0, 6]
    unwritten: Optional[torch.Tensor] = None   # emulation of a mutant that leaves outputs unwritten (True there)


def finish(ar, o):
    """The output tensor (values, in the arithmetic's dtype) of a DwOut."""
    v = o.pre.clamp(0.0, 6.0) if o.relu6 else o.pre
    v = ar.rnd(v)
    if o.unwritten is not None:
        v = torch.where(o.unwritten, torch.full_like(v, CANARY), v)
    return v


def expected(o):
    """r of the gaussian bound: the fp64 output before its rounding."""
    return o.pre.clamp(0.0, 6.0) if o.relu6 else o.pre


def relu6_mask(ar, y):
    """[0 < y < 6] by value (-0.0 is a zero)."""
    lo = y >= 0 if "ge_mask" in ar.mut else y > 0
    hi = y <= 6 if "le6_mask" in ar.mut else y < 6
    return lo & hi


def dw_fwd(ar, x, w9c, bias, stride, relu6):
    """y[b][oh][ow][c] = act(sum x[b][s oh-1+kh][s ow-1+kw][c] w9c[kh*3+kw][c] + bias[c]);  x [B][H][W][C], w9c [9][C]."""
    dt = ar.dtype
    B, H, W, C = x.shape
    OH, OW = out_size(H, stride), out_size(W, stride)
    unwritten = None
    if "oh_floor" in ar.mut and stride == 2 and H > 1:                 # mutant: OH = H / 2, the last row of an odd H is lost
        unwritten = torch.zeros(B, OH, OW, C, dtype=torch.bool, device=x.device)
        unwritten[:, H // 2:] = True
    xp = F.pad(x.to(dt), (0, 0, 1, 1, 1, 1))
    wd = w9c.to(dt)
    acc = torch.zeros(B, OH, OW, C, dtype=dt, device=x.device)
    S = torch.zeros_like(acc) if ar.ref else None
    for kh in range(3):
        for kw in range(3):
            src = xp
            if "drop_border" in ar.mut and kw == 2:                    # mutant: the last input column is out of range
                src = xp.clone()
                src[:, :, W] = 0
            rows = src[:, kh:kh + stride * (OH - 1) + 1:stride, kw:kw + stride * (OW - 1) + 1:stride]
            acc = acc + rows * wd[kh * 3 + kw]
            if ar.ref:
                S += rows.abs() * wd[kh * 3 + kw].abs()
    if bias is not None and "no_bias" not in ar.mut:
        acc = acc + bias.to(dt)
        if ar.ref:
            S += bias.to(dt).abs()
    return DwOut(acc + 0.0, S, bool(relu6), unwritten)


def dw_bwd(ar, g, y, w9c, H, W, stride, relu6):
    """gx[b][h][w][c] = sum (g m)[b][(h+1-kh)/s][(w+1-kw)/s][c] w9c[kh*3+kw][c] over integral, in-range quotients;
    m = [0 < y < 6] if relu6 else 1.  g, y [B][OH][OW][C].  Written as the adjoint scatter: every tap's product is added
    at the input pixels (s oh - 1 + kh, s ow - 1 + kw); per input pixel the taps arrive in ascending order."""
    dt = ar.dtype
    B, OH, OW, C = g.shape
    assert (OH, OW) == (out_size(H, stride), out_size(W, stride))
    gm = g.to(dt)
    if relu6:
        gm = torch.where(relu6_mask(ar, y.to(dt)), gm, torch.zeros_like(gm))
    wd = w9c.to(dt)
    acc = torch.zeros(B, H + 2, W + 2, C, dtype=dt, device=g.device)
    S = torch.zeros_like(acc) if ar.ref else None
    for kh in range(3):
        for kw in range(3):
            tap = 8 - (kh * 3 + kw) if "flip_taps" in ar.mut else kh * 3 + kw
            sl = (slice(None), slice(kh, kh + stride * (OH - 1) + 1, stride), slice(kw, kw + stride * (OW - 1) + 1, stride))
            acc[sl] = acc[sl] + gm * wd[tap]
            if ar.ref:
                S[sl] += gm.abs() * wd[tap].abs()
    crop = lambda a: a[:, 1:H + 1, 1:W + 1].contiguous()
    return DwOut(crop(acc) + 0.0, None if S is None else crop(S), False)


# ---------------------------------------------------------------------------------------------------------- operands
class Operands(NamedTuple):
    x: torch.Tensor              # [B][H][W][C] bf16
    w9c: torch.Tensor            # [9][C] fp32
    bias: Optional[torch.Tensor]  # [C] fp32
    g: torch.Tensor              # [B][OH][OW][C] bf16


def operands(name, leg, B, H, W, C, stride, with_bias=True):
    """leg: 'clamp' / 'rounding' (exact sets) or 'gaussian'.  On the CPU; the GPU tests copy the very same tensors."""
    gen = rng(name, leg)
    OH, OW = out_size(H, stride), out_size(W, stride)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen)
    if leg == "clamp":
        x, w, b, g = ri(-3, 3, B, H, W, C), ri(-2, 2, 9, C), ri(-3, 6, C), ri(-3, 3, B, OH, OW, C)
    elif leg == "rounding":
        x, w, b, g = ri(-127, 127, B, H, W, C), ri(-15, 15, 9, C), ri(-64, 64, C), ri(-127, 127, B, OH, OW, C)
    else:
        rn = lambda *shape: torch.randn(shape, generator=gen)
        x, w, b, g = rn(B, H, W, C), rn(9, C) / 3.0, rn(C), rn(B, OH, OW, C)
    return Operands(x.to(BF16), w.to(F32).contiguous(), b.to(F32) if with_bias else None, g.to(BF16))


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
    """Exact legs, on the reference alone: integer values, sum |terms| < 2^23; clamp set: every output is a bf16 value;
    rounding set: at least 10 % of the outputs are not."""
    worst = float(o.S.max())
    assert worst < 2.0 ** 23, f"{name}: sum |terms| = {worst:.0f} >= 2^23: the exact leg's premise fails"
    assert bool((o.pre == o.pre.round()).all()), f"{name}: the reference is not integer valued"
    inexact = float((bf16_rne(o.pre) != o.pre).double().mean())
    if leg == "clamp":
        assert inexact == 0.0, f"{name}: clamp set values are not all bf16 values ({inexact:.3f})"
    else:
        assert inexact >= 0.10, f"{name}: only {inexact:.3f} of the outputs test the rounding"
    return worst, inexact


def branch_shares(o):
    """Shares of pre <= 0, 0 < pre < 6, pre >= 6."""
    n = o.pre.numel()
    lo, hi = int((o.pre <= 0).sum()), int((o.pre >= 6).sum())
    return lo / n, (n - lo - hi) / n, hi / n


def compare_exact(name, got, o):
    """got: the kernel's (or emulation's) tensor; o: the reference DwOut.  Raises on any bit that differs."""
    want = finish(Arith(), o)
    got = got.reshape(want.shape)
    a, b = bits(got.cpu()), bits(want.cpu())
    if torch.equal(a, b):
        return 0
    bad = (a != b)
    first = tuple(int(v) for v in bad.nonzero()[0])
    raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} outputs differ in bits; first at [b][h][w][c] = {first}: "
                         f"got {float(got[first])}, want {float(want[first])} (exact {float(o.pre[first])})")


def gaussian_ratio(got, o):
    """max over elements of |got - r| / (2^-8 |r| + A (1 + 2^-8))."""
    r = expected(o)
    a = acc_eps(o.S, N_TERMS)
    bound = (2.0 ** -8 * (r.abs() + a) + a).clamp_min(2.0 ** -126)
    return float(((got.reshape(r.shape).double().cpu() - r.cpu()).abs() / bound.cpu()).max())
