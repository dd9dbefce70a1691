"""float64 restatement of the whole-head attention kernels (csrc/adil_attention.hip: adil_attn_fwd / adil_attn_bwd), an fp32
emulation with the kernels' rounding points, mutants, operand generators and comparators, written over
`classifier_reference.Arith`.  Plain torch; no GPU.

    qkv, gqkv [B][T][3][H][64] bf16, o, go [B][T][H][64] bf16, lse [B][H][T] fp32.  For image b, head h, query i, key j < T:
    t_ij = 0.125 sum_d q_id k_jd;  m_i = max_j t_ij;  e_ij = exp(t_ij - m_i);  l_i = sum_j e_ij;  lse_i = m_i + ln l_i
    o_id = bf16((sum_j bf16(e_ij) v_jd) / l_i)
    p_ij = exp(t_ij - lse_i);  dp_ij = sum_d go_id v_jd;  delta_i = sum_d go_id o_id (the stored bf16 o);
    ds_ij = p_ij (dp_ij - delta_i);  gv_jd = bf16(sum_i bf16(p_ij) go_id);
    gq_id = bf16(0.125 sum_j bf16(ds_ij) k_jd);  gk_jd = bf16(0.125 sum_i bf16(ds_ij) q_id)

Legs:

selection   k_j is a +-1 code of j over the 64 dimensions: bit b of j (b = 0 .. 7) as +1 / -1 in dimensions 8b .. 8b+7, so two
            keys differ in at least 8 dimensions and k_a . k_b <= 48 for a != b.  q_i = 128 k_pi(i) for a seeded map pi that
            is NOT injective (T >= 2); v and go are integers of magnitude <= 4.  Then t_{i pi(i)} = 1024 and every other
            t_ij <= 768: exp(-256) is zero in any fp32 implementation, so l = 1, o_i = v_pi(i), gv_j = sum_{pi(i) = j} go_i, and
            dp_{i pi(i)} = delta_i as equal sums of the same integers, hence ds = 0 and gq = gk = 0.  The premises are asserted
            on the reference alone (`exact_references`): the gap is >= 200, every sum of magnitudes stays below 2^24 (so each
            sum is exact in fp32 in any order), the outputs are bf16 values.  o and gqkv are compared BIT FOR BIT (int16, a
            zero of either sign counting as zero); lse under the gaussian leg's bound (its ln / exp round trip is not
            bit-defined).
negative    The same with every real score below -200, so that a padded key that took part with its score of 0 would take
            the whole row.  A component common to all scores cannot be added in the code's own dimensions (the 8 x 8 code
            spans all 64 of them, and g . k_j constant over the keys forces g = 0), so here each bit is repeated 7 times
            (dimensions 7b .. 7b+6: keys differ in >= 7 dimensions, k_a . k_b <= 42 of 56) and dimensions 56 .. 63 hold the
            common component: 1 in every key, -1280 in every query.  t_{i pi(i)} = 896 - 1280 = -384, every other real
            t_ij <= 672 - 1280 = -608: gap 224.  o, gv, gq = gk = 0 are exact as above, lse_i = -384.
gaussian    N(0,1) q, k, v, go (t is then N(0,1) per pair).
peaked      the same with q scaled by 4 (rows dominated by a few keys).

Bounds of the gaussian legs, derived from the rounding points, not fitted to any output.  u = 2^-24 is the unit roundoff of
fp32.  A rounding to bf16 (nearest even) moves v by at most half a unit of its last place, between 2^-9 |v| and 2^-8 |v|
according to the mantissa: the first-order term taken is 2^-9 |v|, and since EVERY bound below is twice its first-order sum
the worst case 2^-8 |v| is covered.  acc_eps(S, n) = 2 n u S bounds the error of n fp32 terms of magnitude sum S accumulated
in any order (classifier_reference).  The doubling also covers all second-order terms.
    t       64 products:  At_ij = 0.125 acc_eps(sum_d |q_id| |k_jd|, 64)  (the factor 0.125 is exact)
    e, p    x = t - m (resp. t - lse): one fp32 subtraction, u |x|; exp as exp2(x log2 e): the rounded constant and the
            rounded product shift the exponent by 2 u |x| log2 e, the hardware exp2 is good to one unit of the last place,
            together (1 + |x|) 2^-23 relative; an error of At in t is a relative error At of exp.  Relative error of e_ij
            (against exp(t_ij - m_i) for the m_i the kernel chose; softmax does not depend on it) and of p_ij:
                E_ij = At_ij + u |x_ij| + (1 + |x_ij|) 2^-23
    l       l_i = L_i (1 + lambda_i), L_i = sum_j exp(t_ij - m_i):  Lam_i = sum_j p_ij E_ij + T u  (the sum of T positive
            terms: relative T u)
    lse     ln l_i = ln L_i + lambda_i; logf to 2 units of the last place; one fp32 addition:
                |lse - r| <= 2 (Lam_i + 2 u |ln L_i| + u |r|)
    o       bf16(e_ij) / l_i = p_ij (1 + E)(1 + 2^-9)/(1 + lambda): with W_id = sum_j p_ij |v_jd| and
            WE_id = sum_j p_ij E_ij |v_jd|,
                first = 2^-9 W + WE + Lam_i W + acc_eps(W, T) + u |r| (the division) + 2^-9 |r| (the rounding of o)
                |o - r| <= 2 first
    gqkv    restated from the kernel's OWN stored o and lse (the same bits on both sides: that removes the forward's
            roundings from the comparison, as the head tests do with `pooled`).  Adp = acc_eps(sum_d |go| |v|, 64),
            Adl = acc_eps(sum_d |go| |o|, 64); ds = p (dp - delta) with one subtraction and one product:
                Dds_ij = p_ij (Adp_ij + Adl_i) + |ds_ij| (E_ij + 2 u)
            gv: first = sum_i p_ij |go_id| (2^-9 + E_ij) + acc_eps(sum_i p_ij |go_id|, T) + 2^-9 |r|
            gq: first = 0.125 (sum_j (2^-9 |ds_ij| + Dds_ij) |k_jd| + acc_eps(sum_j |ds_ij| |k_jd|, T)) + 2^-9 |r|
            gk: the same over i with q.        |g. - r| <= 2 first
    No element is excluded.

Every operation is written once (`attention`) over an `Arith`: fp64 without rounding is the reference; fp32 with the rounding
points above, on tiles padded to 32 tokens as the kernels pad them, is the emulation, which also takes the mutants of
tests/test_attention_cpu.py."""
from typing import NamedTuple, Optional

import torch

from classifier_reference import BF16, CANARY, F32, Arith, acc_eps, bf16_rne, rng  # noqa: F401  (CANARY: re-exported)

F64 = torch.float64
D = 64
TILE = 32
MAX_TOKENS = 256                 # adil_attn_max_tokens() of this build; the tests assert the library says the same

# (B, T, H): one token; the tokens of a 32 x 32 image; an odd size below a tile; a tile edge and one past it; two tiles; the
# network's own T with 24 workgroups (the padding to 224 lives here); the longest sequence.
ROWS = [(1, 1, 1), (2, 5, 2), (1, 17, 3), (2, 32, 1), (1, 33, 2), (1, 64, 2), (2, 197, 12), (1, MAX_TOKENS, 1)]
EXACT_LEGS = ("selection", "negative")
GAUSSIAN_LEGS = ("gaussian", "peaked")
LEGS = EXACT_LEGS + GAUSSIAN_LEGS
MUTANTS = ("no_scale", "scale_twice", "pad_keys", "pad_queries", "no_delta", "ds_transposed", "gk_unscaled", "kv_swapped",
           "next_head", "softmax_query_axis", "lse_m_only")
U = 2.0 ** -24
UB = 2.0 ** -9


class Operands(NamedTuple):
    qkv: torch.Tensor            # [B][T][3 H 64] bf16
    go: torch.Tensor             # [B][T][H 64] bf16
    H: int
    pi: Optional[torch.Tensor]   # exact legs: [B][H][T] the selected key of every query


class Results(NamedTuple):
    o: torch.Tensor              # bf16 [B][T][H 64]
    lse: torch.Tensor            # fp32 [B][H][T]
    gqkv: torch.Tensor           # bf16 [B][T][3 H 64]


def row_name(row, leg):
    return "attention/%s/%s" % (tuple(row), leg)


def codes(T, rep):
    """[T][8 rep]: bit b of j as +1 / -1, repeated rep times."""
    j = torch.arange(T)
    bits = ((j[:, None] >> torch.arange(8)[None, :]) & 1).double() * 2 - 1          # [T][8]
    return bits.repeat_interleave(rep, dim=1)


def operands(name, leg, B, T, H):
    """On the CPU; the GPU tests copy the very same tensors."""
    gen = rng(name, leg)
    if leg in GAUSSIAN_LEGS:
        x = torch.randn((B, T, 3, H, D), generator=gen, dtype=F64)
        if leg == "peaked":
            x[:, :, 0] *= 4.0
        go = torch.randn((B, T, H, D), generator=gen, dtype=F64)
        return Operands(x.reshape(B, T, 3 * H * D).to(BF16).contiguous(), go.reshape(B, T, H * D).to(BF16).contiguous(), H, None)
    pi = torch.randint(0, T, (B, H, T), generator=gen)
    if T >= 2:
        pi[..., 1] = pi[..., 0]                                           # not injective, whatever the draw
    k = torch.ones(T, D, dtype=F64)
    if leg == "selection":
        k[:] = codes(T, 8)
    else:
        k[:, :56] = codes(T, 7)
    q = 128.0 * k[pi]                                                     # [B][H][T][64]
    if leg == "negative":
        q[..., 56:] = -1280.0
    x = torch.zeros(B, T, 3, H, D, dtype=F64)
    x[:, :, 0] = q.permute(0, 2, 1, 3)
    x[:, :, 1] = k[None, :, None, :]
    x[:, :, 2] = torch.randint(-4, 5, (B, T, H, D), generator=gen).double()
    go = torch.randint(-4, 5, (B, T, H, D), generator=gen).double()
    return Operands(x.reshape(B, T, 3 * H * D).to(BF16).contiguous(), go.reshape(B, T, H * D).to(BF16).contiguous(), H, pi)


# ------------------------------------------------------------------------------------------------------------ operations
def heads_of(x, H, sections):
    """[B][T][sections H 64] -> [B][sections][H][T][64]"""
    B, T, _ = x.shape
    return x.reshape(B, T, sections, H, D).permute(0, 2, 3, 1, 4)


def rows_of(x):
    """[B][sections][H][T][64] -> [B][T][sections H 64]"""
    B, S, H, T, _ = x.shape
    return x.permute(0, 3, 1, 2, 4).reshape(B, T, S * H * D)


def _pad(x, Tp, clamp):
    """rows T .. Tp-1 behind [..., T, :]: zeros, or copies of the last row (the `pad_queries` mutant)."""
    T = x.shape[-2]
    if Tp == T:
        return x
    tail = x[..., T - 1:T, :].expand(*x.shape[:-2], Tp - T, x.shape[-1]) if clamp else x.new_zeros(*x.shape[:-2], Tp - T, x.shape[-1])
    return torch.cat([x, tail], dim=-2)


def attention(ar, qkv, go, H, stored=None):
    """Forward and input gradient from the stored bf16 operands.  `stored` = (o, lse) of the implementation under test: the
    gradient is then restated from them.  Returns Results in the arithmetic's dtype (values; the callers cast)."""
    mut, dt = ar.mut, ar.dtype
    B, T, _ = qkv.shape
    rnd = (lambda v: v) if ar.ref else ar.rnd
    x = heads_of(qkv.to(dt), H, 3)
    if "next_head" in mut:                                               # mutant: head h reads the columns of head h + 1
        x = x.roll(-1, dims=2)
    sk, sv = (2, 1) if "kv_swapped" in mut else (1, 2)                   # mutant: k and v sections swapped
    Tp = T if ar.ref else (T + TILE - 1) // TILE * TILE
    clamp = "pad_queries" in mut                                         # mutant: padded query rows repeat row T-1 and count
    q, k, v = _pad(x[:, 0], Tp, clamp), _pad(x[:, sk], Tp, False), _pad(x[:, sv], Tp, False)
    g = _pad(heads_of(go.to(dt), H, 1)[:, 0], Tp, clamp)
    scale = 1.0 if "no_scale" in mut else (0.125 * 0.125 if "scale_twice" in mut else 0.125)
    real = torch.arange(Tp) < T
    keyok = torch.ones(Tp, dtype=torch.bool) if "pad_keys" in mut else real   # mutant: padded keys take part with score 0
    qok = torch.ones(Tp, dtype=torch.bool) if clamp else real
    t = (q @ k.transpose(-1, -2)) * scale                                # [B][H][Tp][Tp]
    tm = t.masked_fill(~keyok[None, None, None, :], float("-inf"))
    col = "softmax_query_axis" in mut                                    # mutant: softmax over the query axis
    axis = -2 if col else -1
    m = tm.amax(axis, keepdim=True)
    e = torch.exp(tm - m)
    l = e.sum(axis, keepdim=True)
    lse = (m if "lse_m_only" in mut else m + torch.log(l)).squeeze(axis)  # mutant: lse = m
    o = rnd(rnd(e / l) @ v) if col else rnd((rnd(e) @ v) / l)
    if stored is not None:
        o_b = _pad(heads_of(stored[0].to(dt), H, 1)[:, 0], Tp, clamp)
        lse_b = _pad(stored[1].to(dt)[..., None], Tp, clamp)[..., 0]
    else:
        o_b, lse_b = (o if ar.ref else bf16_rne(o)), lse
    p = torch.exp(t - (lse_b[..., None, :] if col else lse_b[..., :, None]))
    p = torch.where(keyok[None, None, None, :] & qok[None, None, :, None], p, torch.zeros_like(p))
    dp = g @ v.transpose(-1, -2)
    delta = torch.zeros_like(lse_b) if "no_delta" in mut else (g * o_b).sum(-1)   # mutant: delta missing
    ds = p * (dp - delta[..., :, None])
    dsu = ds.transpose(-1, -2) if "ds_transposed" in mut else ds        # mutant: dS transposed
    gv = rnd(rnd(p).transpose(-1, -2) @ g)
    gq = rnd(scale * (rnd(dsu) @ k))
    gk = rnd((1.0 if "gk_unscaled" in mut else scale) * (rnd(dsu).transpose(-1, -2) @ q))   # mutant: gk unscaled
    sect = [gq, None, None]
    sect[sk], sect[sv] = gk, gv
    gx = torch.stack([s[..., :T, :] for s in sect], dim=1)              # [B][3][H][T][64]
    if "next_head" in mut:
        gx = gx.roll(1, dims=2)
    return Results(rows_of(o[:, None, :, :T]), lse[..., :T], rows_of(gx))


def cast(r):
    return Results(r.o.to(BF16), r.lse.float(), r.gqkv.to(BF16))


def emulate(op, mut=(), stored=None):
    """The fp32 emulation of both kernels (with mutants), outputs in their storage types."""
    return cast(attention(Arith(F32, 16, mut), op.qkv, op.go, op.H, stored))


# ------------------------------------------------------------------------------------------------------------ comparators
def exact_references(name, leg, B, T, H):
    """Operands and the one correct value of o and gqkv (lse: the value the bound is taken around); every premise is
    asserted on the reference alone."""
    op = operands(name, leg, B, T, H)
    x = heads_of(op.qkv.double(), H, 3)
    q, k, v = x[:, 0], x[:, 1], x[:, 2]
    g = heads_of(op.go.double(), H, 1)[:, 0]
    t = 0.125 * (q @ k.transpose(-1, -2))
    assert float((q.abs() @ k.abs().transpose(-1, -2)).max()) < 2.0 ** 24, f"{name}: sum |q| |k| >= 2^24"
    best = 1024.0 if leg == "selection" else -384.0
    sel = torch.zeros_like(t, dtype=torch.bool).scatter_(-1, op.pi[..., None], True)
    assert bool((t[sel] == best).all()), f"{name}: the selected score is not {best}"
    if T > 1:
        assert float(t[~sel].max()) <= best - 200.0, f"{name}: gap {best - float(t[~sel].max())} < 200"
    if leg == "negative":
        assert float(t.max()) < -200.0, f"{name}: a real score is not below -200"
    if T >= 2:
        assert bool((op.pi[..., 0] == op.pi[..., 1]).all()), f"{name}: pi is injective"
    want = cast(attention(Arith(), op.qkv, op.go, H))                    # exp(-224) is 1e-98 in fp64: gone in the cast
    o = torch.gather(v, 2, op.pi[..., None].expand(-1, -1, -1, D))
    gv = torch.zeros_like(v).scatter_add_(2, op.pi[..., None].expand(-1, -1, -1, D), g)
    gx = torch.stack([torch.zeros_like(gv), torch.zeros_like(gv), gv], dim=1)
    for what, a, b in (("o", want.o, rows_of(o[:, None])), ("gqkv", want.gqkv, rows_of(gx))):
        assert bool((bf16_rne(b) == b).all()), f"{name}: {what} holds values that are no bf16 values"
        assert torch.equal(a.double() + 0.0, b + 0.0), f"{name}: the fp64 restatement's {what} is not the selection's closed form"
    assert float((g.abs() @ v.abs().transpose(-1, -2)).max()) < 2.0 ** 24 and float(gv.abs().max()) < 2.0 ** 24
    assert bool((want.lse == best).all()), f"{name}: lse is not {best}"
    return op, want


def _bits(t):
    """int16 view of bf16, with -0.0 counted as +0."""
    t = t.detach().cpu().contiguous()
    t = torch.where(t == 0, torch.zeros_like(t), t)
    return t.view(torch.int16)


def compare_bits(name, got, want):
    """Raises on any bit that differs (a zero of either sign counts as zero)."""
    assert got.dtype == want.dtype == BF16, (name, got.dtype, want.dtype)
    got = got.reshape(want.shape)
    a, b = _bits(got), _bits(want)
    if torch.equal(a, b):
        return 0
    bad = a != b
    first = tuple(int(v) for v in bad.nonzero()[0])
    raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} outputs differ in bits; first at {first}: "
                         f"got {float(got.cpu()[first])}, want {float(want[first])}")


def _ratio(got, r, bound):
    got = got.double().cpu().reshape(r.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - r).abs() / bound.clamp_min(2.0 ** -126)).max())


def ratios(op, got):
    """max |got - r| / bound of o, lse and gqkv (gqkv restated from got.o and got.lse) against fp64.  Returns the three."""
    H = op.H
    B, T, _ = op.qkv.shape
    x = heads_of(op.qkv.double(), H, 3)
    q, k, v = x[:, 0], x[:, 1], x[:, 2]
    g = heads_of(op.go.double(), H, 1)[:, 0]
    kt, vt = k.transpose(-1, -2), v.transpose(-1, -2)
    ref = attention(Arith(), op.qkv, op.go, H)
    t = 0.125 * (q @ kt)
    At = 0.125 * acc_eps(q.abs() @ k.abs().transpose(-1, -2), D)
    # ---- forward, against the true softmax
    xm = t - t.amax(-1, keepdim=True)
    p = torch.softmax(t, -1)
    E = At + U * xm.abs() + (1 + xm.abs()) * 2.0 ** -23
    Lam = (p * E).sum(-1) + T * U                                        # [B][H][T]
    lnL = torch.log(torch.exp(xm).sum(-1))
    r_lse = ref.lse
    b_lse = 2 * (Lam + 2 * U * lnL.abs() + U * r_lse.abs())
    r_o = heads_of(ref.o, H, 1)[:, 0]
    W = p @ v.abs()
    first = UB * W + (p * E) @ v.abs() + Lam[..., None] * W + acc_eps(W, T) + U * r_o.abs() + UB * r_o.abs()
    ro = _ratio(heads_of(got.o.cpu(), H, 1)[:, 0], r_o, 2 * first)
    rl = _ratio(got.lse, r_lse, b_lse)
    # ---- gradient, restated from the stored o and lse
    o_s = heads_of(got.o.cpu().double(), H, 1)[:, 0]
    lse_s = got.lse.cpu().double().reshape(B, H, T)
    rg = float("inf")
    if bool(torch.isfinite(o_s).all()) and bool(torch.isfinite(lse_s).all()):
        refb = attention(Arith(), op.qkv, op.go, H, stored=(got.o.cpu(), got.lse.cpu().reshape(B, H, T)))
        xb = t - lse_s[..., None]
        pb = torch.exp(xb)
        Eb = At + U * xb.abs() + (1 + xb.abs()) * 2.0 ** -23
        dp = g @ vt
        delta = (g * o_s).sum(-1)
        ds = pb * (dp - delta[..., None])
        Adp = acc_eps(g.abs() @ v.abs().transpose(-1, -2), D)
        Adl = acc_eps((g.abs() * o_s.abs()).sum(-1), D)
        Dds = pb * (Adp + Adl[..., None]) + ds.abs() * (Eb + 2 * U)
        r = heads_of(refb.gqkv, H, 3)
        Wv = pb.transpose(-1, -2) @ g.abs()
        f_v = (pb * (UB + Eb)).transpose(-1, -2) @ g.abs() + acc_eps(Wv, T) + UB * r[:, 2].abs()
        f_q = 0.125 * ((UB * ds.abs() + Dds) @ k.abs() + acc_eps(ds.abs() @ k.abs(), T)) + UB * r[:, 0].abs()
        f_k = 0.125 * ((UB * ds.abs() + Dds).transpose(-1, -2) @ q.abs() + acc_eps(ds.abs().transpose(-1, -2) @ q.abs(), T)) \
            + UB * r[:, 1].abs()
        bound = 2 * torch.stack([f_q, f_k, f_v], dim=1)
        rg = _ratio(heads_of(got.gqkv.cpu(), H, 3), r, bound)
    return ro, rl, rg


def lse_ratio(op, got_lse, want_lse):
    """Exact legs: lse under the gaussian leg's bound around its exact value."""
    H = op.H
    B, T, _ = op.qkv.shape
    x = heads_of(op.qkv.double(), H, 3)
    q, k = x[:, 0], x[:, 1]
    t = 0.125 * (q @ k.transpose(-1, -2))
    At = 0.125 * acc_eps(q.abs() @ k.abs().transpose(-1, -2), D)
    xm = t - t.amax(-1, keepdim=True)
    E = At + U * xm.abs() + (1 + xm.abs()) * 2.0 ** -23
    Lam = (torch.softmax(t, -1) * E).sum(-1) + T * U
    r = want_lse.double()
    return _ratio(got_lse, r, 2 * (Lam + U * r.abs()))


def check(name, leg, op, got, want=None):
    """Raises unless `got` (Results in storage types) passes the leg.  Prints the ratios it asserts."""
    if leg in EXACT_LEGS:
        compare_bits(name + "/o", got.o.cpu(), want.o)
        compare_bits(name + "/gqkv", got.gqkv.cpu(), want.gqkv)
        rl = lse_ratio(op, got.lse, want.lse)
        print(name, "lse |err| / bound %.3f" % rl)
        assert rl <= 1.0, f"{name}: lse is {rl:.3g} bounds from its value"
    else:
        ro, rl, rg = ratios(op, got)
        print(name, "max |err| / bound: o %.3f lse %.3f gqkv %.3f" % (ro, rl, rg))
        assert ro <= 1.0 and rl <= 1.0 and rg <= 1.0, f"{name}: max |err| / bound: o {ro:.3g} lse {rl:.3g} gqkv {rg:.3g}"


_cache = {}


def case(row, leg):
    """(name, op, want): computed once per process and shared, never modified."""
    key = (tuple(row), leg)
    if key not in _cache:
        name = row_name(row, leg)
        if leg in EXACT_LEGS:
            op, want = exact_references(name, leg, *row)
        else:
            op, want = operands(name, leg, *row), None
        _cache[key] = (name, op, want)
    return _cache[key]
