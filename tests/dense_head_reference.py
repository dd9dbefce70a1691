"""float64 restatement of the pooled head kernels behind an eval-BatchNorm + ReLU (csrc/adil_head.hip: adil_bn_pool_head_fwd /
adil_bn_pool_head_bwd), an fp32 emulation, operand generators and comparators, over `classifier_reference.Arith` and the
operations of tests/head_reference.py.  Plain torch; CPU or GPU.

    prologue   pre[b][hw][c] = f32(f32(f32(x) * pscale[c]) + pshift[c]): two fp32 roundings, no fma;
               p = pre > 0 ? pre : +0 (never rounded to bf16)
    forward    S[b][c] = sum_hw p;  pooled = f32(S * inv_hw), inv_hw = 1.0f / (float)HW;
               logits[b][n] = bias[n] + sum_c pooled[b][c] w[n][c]
    gradient   gpooled[b][c] = sum_n g[b][n] w[n][c];  v[b][c] = f32(f32(gpooled * inv_hw) * pscale[c]);
               gx[b][hw][c] = bf16(v[b][c]) where pre[b][hw][c] > 0, +0 elsewhere

pre, p and the mask are BIT-DEFINED: they are restated in fp32 on both sides (the reference and the emulation), as
tests/dense1x1_reference.py does for the same prologue; the reference then sums the fp32 values p in fp64.

exact leg     pscale in {+-1/2, +-1, +-2} (half of the channels negative), pshift an integer in [-4, 4], and
              x = (T - pshift) / pscale for an integer target pre-activation T: a bf16 value (asserted), and pre == T
              exactly (asserted).  For a power-of-two HW, 40 % of the elements of every row of 8 channels (the 8 channels
              of a lane) are given T in [-4, 0] (at least one of them 0) and the others T in [1, 4], resp. [1, 6] for
              HW >= 64, so that S, and with it pooled, needs more than 8 bits.  For any other HW the post-ReLU values are
              k + d with sum_hw d = 0, k in [2, 4]: the pixels come in pairs d = (+e, -e); 60 % of the pairs of a row of 8
              channels have e = k, and their -k partner gets T in [-3, 0] instead of 0: it is masked, contributes 0 and
              S = HW k still holds (`head_reference.assert_pool_identity` is the premise for these HW).  w, bias, g as in
              head_reference.  The premises of head_reference.exact_references are asserted for the new S, and so are the
              share of masked elements (20 % .. 80 %, in every row of 8 channels too), the presence of pre == 0 and that
              both signs of pscale occur among masked and unmasked elements.  pooled, logits, gpooled and gx have ONE
              correct value each and are compared bit for bit, a zero of either sign counting as zero.
gaussian leg  N(0,1) x, w, bias, g; |pscale| uniform in [0.5, 1.5] with random signs; pshift N(0,1).  In the channels
              c % 8 == 3, x = +-c_k (a bf16 value in [1, 2)) and pshift = -f32(c_k * pscale): where x = +c_k, pre is exactly
              0 under the two specified roundings, and a contracted fma leaves the product's rounding error as a residual
              (positive for about half of the channels: the branch flips).  Bounds: head_reference's with the terms p in
              place of x,
                  |pooled - S / HW| <= A / HW + 2 u (|S| / HW + A / HW),   A = acc_eps(sum p, HW);
              logits and gpooled are restated from the kernel's own stored pooled resp. from g with head_reference's
              bounds; gx is a bit-defined function of the stored gpooled, x and the tables and is compared bit for bit.  No
              element is excluded."""
from typing import NamedTuple, Optional

import torch

import head_reference as href
from classifier_reference import BF16, CANARY, F32, Arith, rng  # noqa: F401  (CANARY: re-exported to the tests)
from head_reference import Results, compare_bits, compare_exact, is_pow2  # noqa: F401

F64 = torch.float64
# (B, HW, C, N): head_reference's rows, the network's head at 64 x 64 (2 x 2 pixels, 1024 channels, 1000 classes) and the
# network's head at 224 x 224 with a few classes
ROWS = list(href.ROWS) + [(2, 4, 1024, 1000), (2, 49, 1024, 12)]
NAN_ROWS = [(3, 49, 24, 10), (17, 9, 40, 7)]
MUTANTS = ("fma", "mask_on_x", "mask_ge", "no_relu", "relu_after_pool", "pre_bf16", "no_pscale_in_gx", "scale_before_inv_hw",
           "shift_ignored", "drop_last", "trunc")
ZERO_CHANNEL = 3                 # gaussian leg: the channels c % 8 == 3 hold pre == 0


class Operands(NamedTuple):
    x: torch.Tensor              # [B][HW][C] bf16
    pscale: torch.Tensor         # [C] fp32
    pshift: torch.Tensor         # [C] fp32
    w: torch.Tensor              # [N][C] fp32
    bias: torch.Tensor           # [N] fp32
    g: torch.Tensor              # [B][N] fp32
    k: Optional[torch.Tensor]    # exact leg, HW no power of two: the integer mean [B][C]


def _chosen(gen, n, share):
    """A boolean [n] with exactly ceil(share n) entries set, at random places."""
    m = torch.zeros(n, dtype=torch.bool)
    m[torch.randperm(n, generator=gen)[:(int(share * 10) * n + 9) // 10]] = True
    return m


def _rows_of_8(flag_bhwc):
    """[B][HW][C] -> [C / 8][B HW 8]: the elements of each row of 8 channels (what one lane owns, over the batch)."""
    B, HW, C = flag_bhwc.shape
    return flag_bhwc.reshape(B, HW, C // 8, 8).permute(2, 0, 1, 3).reshape(C // 8, B * HW * 8)


def _from_rows_of_8(rows, B, HW, C):
    return rows.reshape(C // 8, B, HW, 8).permute(1, 2, 0, 3).reshape(B, HW, C)


def exact_targets(gen, B, HW, C):
    """Integer target pre-activations T [B][HW][C] (fp64) and, for an HW that is no power of two, the mean k [B][C]."""
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).double()
    G = C // 8
    if is_pow2(HW):
        n = B * HW * 8
        masked = torch.stack([_chosen(gen, n, 0.4) for _ in range(G)])
        tm = torch.where(masked, ri(-4, 0, G, n), ri(1, 4 if HW < 64 else 6, G, n))
        tm[torch.arange(G), masked.double().argmax(1)] = 0.0            # pre == 0 exists in every row of 8 channels
        return _from_rows_of_8(tm, B, HW, C), None
    k = ri(2, 4, B, C)
    P = HW // 2
    n = B * P * 8
    full = _from_rows_of_8(torch.stack([_chosen(gen, n, 0.6) for _ in range(G)]), B, P, C)      # pairs with e = k
    e = torch.where(full, k[:, None, :].expand(B, P, C), ri(-2, 2, B, P, C))
    below = ri(-3, 0, B, P, C)                                          # the masked partner's own pre-activation
    T = k[:, None, :].expand(B, HW, C).clone()                          # an odd HW keeps one pixel at d = 0
    T[:, 0:2 * P:2] = k[:, None, :] + e
    T[:, 1:2 * P:2] = torch.where(full, below, k[:, None, :] - e)
    return T[:, torch.randperm(HW, generator=gen)], k


def operands(name, leg, B, HW, C, N):
    """leg 'exact' or 'gaussian'.  On the CPU; the GPU tests copy the very same tensors."""
    gen = rng(name, leg)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).double()
    sign = torch.ones(C, dtype=F64)
    sign[torch.randperm(C, generator=gen)[:C // 2]] = -1.0
    k = None
    if leg == "exact":
        pscale = sign * 2.0 ** ri(-1, 1, C)
        pshift = ri(-4, 4, C)
        T, k = exact_targets(gen, B, HW, C)
        x = (T - pshift) / pscale
        assert torch.equal(x.to(BF16).double(), x), f"{name}: x is no bf16 value"
        w, bias, g = ri(-4, 4, N, C), ri(-4, 4, N), ri(-4, 4, B, N)
        op = Operands(x.to(BF16).contiguous(), pscale.float(), pshift.float(), w.float(), bias.float(), g.float(), k)
        assert torch.equal(pre_of(Arith(), op.x, op.pscale, op.pshift).double(), T), f"{name}: pre is not the target"
        return op
    rn = lambda *shape: torch.randn(shape, generator=gen)
    x, w, bias, g = rn(B, HW, C).to(BF16), rn(N, C), rn(N), rn(B, N)
    pscale = (sign * (0.5 + torch.rand(C, generator=gen).double())).float()
    pshift = rn(C).float()
    zc = torch.arange(ZERO_CHANNEL, C, 8)
    ck = (1.0 + torch.rand(len(zc), generator=gen)).to(BF16)
    flip = (torch.randint(0, 2, (B, HW, len(zc)), generator=gen) * 2 - 1).to(BF16)
    x[:, :, zc] = flip * ck
    pshift[zc] = -(ck.float() * pscale[zc])
    return Operands(x.contiguous(), pscale.contiguous(), pshift.contiguous(), w.float().contiguous(), bias.float().contiguous(),
                    g.float().contiguous(), None)


# ------------------------------------------------------------------------------------------------------------ operations
def pre_of(ar, x, pscale, pshift):
    """fp32 on both sides: f32(f32(x * pscale) + pshift).  Mutants: one fma; the shift left out."""
    x32, ps, pb = ar.f32(x), ar.f32(pscale).to(x.device), ar.f32(pshift).to(x.device)   # the real values over `Unrounded`
    if "fma" in ar.mut:                                                 # the product is not rounded
        return ar.f32(x32.double() * ps.double() + pb.double())
    if "shift_ignored" in ar.mut:
        return x32 * ps
    return x32 * ps + pb


def mask_of(ar, x, pre):
    if "mask_on_x" in ar.mut:                                           # the sign of x, not of the pre-activation
        return x.float() > 0
    if "mask_ge" in ar.mut:                                             # pre == 0 keeps the gradient
        return pre >= 0
    return pre > 0


def post_of(ar, pre):
    """p [B][HW][C] fp32: pre where pre > 0, +0 elsewhere (the forward's own branch, whatever the gradient's mask mutant)."""
    if "no_relu" in ar.mut or "relu_after_pool" in ar.mut:
        return pre
    p = torch.where(pre > 0, pre, torch.zeros_like(pre))
    if "pre_bf16" in ar.mut:                                            # p rounded to bf16 before the sum
        p = href.bf16_rne(p)
    return p


def pooled_of(ar, p, HW):
    """pooled [B][C] fp32 and (reference) S, sum |p| in fp64."""
    S, Sabs = href.pool_sum(ar, p)
    pooled = href.scale_f32(S, HW, ar)
    if "relu_after_pool" in ar.mut:
        pooled = torch.where(pooled > 0, pooled, torch.zeros_like(pooled))
    return pooled, S, Sabs


def gx_of(ar, gpooled, x, pscale, pshift):
    """[B][HW][C] bf16 from the STORED fp32 gpooled: two fp32 multiplies in the specified order, one rounding, the mask."""
    HW = x.shape[1]
    ps = ar.f32(pscale).to(gpooled.device)
    if "no_pscale_in_gx" in ar.mut:
        v = href.scale_f32(gpooled, HW, ar)
    elif "scale_before_inv_hw" in ar.mut:
        v = href.scale_f32(ar.f32(gpooled) * ps, HW, ar)
    else:
        v = href.scale_f32(gpooled, HW, ar) * ps
    v = ar.rnd(v)
    v = v if isinstance(ar, href.Unrounded) else v.bfloat16()          # over `Unrounded` alone: the real product
    m = mask_of(ar, x, pre_of(ar, x, pscale, pshift))
    return torch.where(m, v[:, None, :].expand(m.shape), torch.zeros((), dtype=v.dtype, device=v.device)).contiguous()


def emulate(op, mut=()):
    """The fp32 emulation of both kernels (with mutants)."""
    ar = Arith(F32, href.GEMM_K, mut)
    HW = op.x.shape[1]
    pooled, _, _ = pooled_of(ar, post_of(ar, pre_of(ar, op.x, op.pscale, op.pshift)), HW)
    logits, _ = href.logits_of(ar, pooled, op.w, op.bias)
    gp, _ = href.gpooled_of(ar, op.g, op.w)
    return Results(pooled.float(), logits.float(), gp.float(), gx_of(ar, gp.float(), op.x, op.pscale, op.pshift))


# ------------------------------------------------------------------------------------------------------------ comparators
def assert_mask_premises(name, op):
    """On the reference alone: the masked share overall and in every row of 8 channels, pre == 0, both signs of pscale on
    both sides of the mask."""
    pre = pre_of(Arith(), op.x, op.pscale, op.pshift)
    masked = ~(pre > 0)
    share = float(masked.double().mean())
    rows = _rows_of_8(masked).double().mean(1)
    assert 0.2 <= share <= 0.8, f"{name}: {share:.2f} of the elements are masked"
    assert 0.2 <= float(rows.min()) and float(rows.max()) <= 0.8, f"{name}: masked share of a row of 8 channels {float(rows.min()):.2f} .. {float(rows.max()):.2f}"
    assert bool((pre == 0).any()), f"{name}: no element with pre == 0"
    neg = (op.pscale < 0)[None, None, :].expand(masked.shape)
    for m in (masked, ~masked):
        assert bool((m & neg).any()) and bool((m & ~neg).any()), f"{name}: one sign of pscale is missing on one side of the mask"
    return share, float((pre == 0).double().mean())


def exact_references(name, B, HW, C, N):
    """Operands and the one correct value of each of the four outputs; every premise asserted on the reference alone."""
    op = operands(name, "exact", B, HW, C, N)
    ar = Arith()
    share, zeros = assert_mask_premises(name, op)
    pooled, S, Sabs = pooled_of(ar, post_of(ar, pre_of(ar, op.x, op.pscale, op.pshift)), HW)
    assert float(Sabs.max()) < 2.0 ** 23, f"{name}: sum |p| >= 2^23"
    assert bool((S == S.round()).all())
    if is_pow2(HW):
        q = 1.0 / HW
    else:
        q = 1.0
        assert torch.equal(S, op.k * HW), f"{name}: the deviations do not cancel"
        href.assert_pool_identity(name, HW, op.k)
    assert bool((pooled.double() == S / HW).all()), f"{name}: pooled is not S / HW"
    logits, Sl = href.logits_of(ar, pooled, op.w, op.bias)
    assert float(Sl.max()) < 2.0 ** 23 * q, f"{name}: |pooled| @ |w| + |bias| = {float(Sl.max()) / q:.0f} quanta >= 2^23"
    assert bool((logits / q == (logits / q).round()).all()), f"{name}: the logits are no multiple of the quantum"
    gp, Sg = href.gpooled_of(ar, op.g, op.w)
    assert float(Sg.max()) < 2.0 ** 23, f"{name}: |g| @ |w| >= 2^23"
    assert bool((gp == gp.round()).all())
    gp32 = gp.float()
    print(name, "masked %.2f, pre == 0 %.3f; sum |terms| in quanta: pool %.0f logits %.0f gpooled %.0f; pooled values that are "
          "no bf16 values %.2f" % (share, zeros, float(Sabs.max()), float(Sl.max()) / q, float(Sg.max()),
                                   float((href.bf16_rne(pooled) != pooled).double().mean())))
    return op, Results(pooled, logits.float(), gp32, gx_of(ar, gp32, op.x, op.pscale, op.pshift))


def gaussian_ratios(name, op, got):
    """max |got - r| / bound of pooled, logits (from got.pooled) and gpooled; gx bit for bit from got.gpooled.  Returns the
    three ratios."""
    ar = Arith()
    B, HW, C = op.x.shape
    u = 2.0 ** -24
    _, S, Sabs = pooled_of(ar, post_of(ar, pre_of(ar, op.x, op.pscale, op.pshift)), HW)
    r, a = S / HW, href.acc_eps(Sabs, HW) / HW
    rp = href._ratio(got.pooled, r, a + 2 * u * (r.abs() + a))
    rl_ref, Sl = href.logits_of(ar, got.pooled.cpu(), op.w, op.bias)
    rl = href._ratio(got.logits, rl_ref, href.acc_eps(Sl, C + 1))
    rg_ref, Sg = href.gpooled_of(ar, op.g, op.w)
    rg = href._ratio(got.gpooled, rg_ref, href.acc_eps(Sg, op.w.shape[0]))
    compare_bits(name + "/gx", got.gx, gx_of(ar, got.gpooled.cpu(), op.x, op.pscale, op.pshift))
    return rp, rl, rg


def row_name(row, leg):
    return "dense_head/%s/%s" % (tuple(row), leg)
