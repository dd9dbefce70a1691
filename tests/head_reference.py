"""float64 restatement of the pooled fp32 head kernels (csrc/adil_head.hip: adil_pool_head_fwd / adil_pool_head_bwd), an
fp32 emulation, operand generators and comparators, written over `classifier_reference.Arith`.  Plain torch; CPU or GPU.

    forward    S[b][c] = sum_hw x[b][hw][c];  pooled = f32(S * inv_hw), inv_hw = 1.0f / (float)HW;
               logits[b][n] = bias[n] + sum_c pooled[b][c] w[n][c]
    gradient   gpooled[b][c] = sum_n g[b][n] w[n][c];  gx[b][hw][c] = bf16(f32(gpooled[b][c] * inv_hw)) for every hw

x and gx are [B][HW][C] bf16; w [N][C], bias [N], g and logits [B][N], pooled and gpooled [B][C] are fp32.  The factors of
every product are the stored fp32 values themselves.  Two operand sets:

exact leg     x, w, g are integers of magnitude <= 4 (bf16 values), bias is an integer.  For a power-of-two HW (1 included) x
              is drawn freely (from [-1, 4] for HW >= 64, so that S, and with it pooled, needs more than the 8 bits of a
              bf16 value): S is an integer below 2^24 whatever the order, and S * inv_hw is exact, a multiple of
              q = 1 / HW.  For any other HW, x[b][hw][c] = k[b][c] + d[b][hw][c] with sum_hw d = 0 (k in [-2, 2], d in
              [-2, 2]): S = HW k exactly, and the premise  f32(f32(HW k) * f32(1 / HW)) == k  is asserted on the reference
              alone (`assert_pool_identity`; it holds for HW in {9, 12, 25, 49, 100} and every integer and quarter-integer
              |k| <= 4096, which tests/test_head_cpu.py checks), so pooled = k, q = 1.  Either way every product
              pooled * w and every partial sum of the logits in ANY order, the bias at any position, is a multiple of q
              below 2^23 q (asserted: |pooled| @ |w|^T + |bias| < 2^23 q), hence exact in fp32; g @ w is a sum of integers
              (asserted: |g| @ |w| < 2^23).  pooled, logits and gpooled therefore have ONE correct value; gx is a
              bit-defined function of gpooled (one fp32 multiply by the fp32 constant inv_hw, one rounding to nearest
              even).  All four are compared BIT FOR BIT, fp32 as int32 and bf16 as int16, a zero of either sign counting as
              zero.
gaussian leg  N(0,1) operands.  Elementwise bounds, derived, not measured.  u = 2^-24 is the unit roundoff of fp32.  A sum of
              n fp32 terms t_i (products included: each is rounded once, or not at all when it is fused) accumulated in any
              order is within gamma_n sum |t_i| of the exact sum, gamma_n = n u / (1 - n u) <= 1.004 n u for n <= 65536; the
              bound used is twice the first-order term,
                  A = acc_eps(sum |t_i|, n) = 2 n 2^-24 sum |t_i|,
              which covers gamma_n, a fused or an unfused multiply-add and every second-order term below.  Every further
              fp32 operation on a value v within A of its exact value r adds one relative rounding: u (|r| + A).
                  pooled   terms x[b][hw][c] (bf16 values, exact in fp32), n = HW: the sum is within A of S.  Then two more
                           roundings, that of the constant 1 / HW itself and that of the multiply, both relative to S / HW:
                               |pooled - S / HW| <= A / HW + 2 u (|S| / HW + A / HW)
                  logits   restated from the kernel's OWN stored pooled (the same fp32 bits on both sides, as
                           classifier_reference does for outputs that are rounded twice): terms pooled[b][c] w[n][c] and
                           bias[n], n = C + 1; the bias add is one of the n additions wherever it sits:
                               |logits - r| <= A,   r = bias + pooled @ w^T in fp64
                  gpooled  terms g[b][n] w[n][c], n = N:   |gpooled - r| <= A,   r = g @ w in fp64
                  gx       a bit-defined function of the kernel's own stored gpooled: compared bit for bit in this leg too.
              No element is excluded.

Every operation is written once over an `Arith`: fp64 with one matmul per GEMM is the reference; fp32 with the pixels summed
in the kernel's order (8 interleaved rows, then the rows in order) and the GEMMs accumulated in 16-wide chunks is the CPU
emulation of the kernels, which also takes the mutants of tests/test_head_cpu.py."""
from typing import NamedTuple, Optional

import torch

from classifier_reference import BF16, CANARY, F32, Arith, Unrounded, bf16_rne, rng  # noqa: F401  (CANARY: re-exported to the tests)

F64 = torch.float64
POOL_ROWS = 8                    # pixel rows of a pooling workgroup (hw = r, r + 8, ...)
POOL_CHANNELS = 256              # channels of a pooling workgroup
GEMM_TILE, GEMM_K = 64, 16       # output tile edge and K step of the head GEMM

# (B, HW, C, N).  The six rows the kernels' contract names: both extents of C; C = 24 / 40, which no channel tile
# divides; HW = 1, a power of two, 49; N = 1, N % 4 != 0, N = 1000; B = 67, which no image tile divides (and which crosses
# the GEMM's 64-row tile).  Then the edges of this tiling: HW = 100 = 3 x 32 + 4 (the four-deep load loop and its tail; HW < 8
# leaves pixel rows idle), HW = 1024 (a power of two whose pooled values need more than 8 bits), C = 264 (one 16-byte chunk
# past a 256-channel workgroup), N = 65 (one column past a 64-wide GEMM tile, on the element-wise path), N = 68 (the same on
# the 16-byte path).
ROWS = [(1, 1, 8, 1), (3, 49, 24, 10), (17, 9, 40, 7), (2, 16, 1280, 1000), (2, 4, 2048, 12), (67, 49, 64, 4),
        (5, 100, 264, 65), (2, 1024, 8, 5), (3, 12, 72, 68)]
NAN_ROWS = [(3, 49, 24, 10), (17, 9, 40, 7)]
IDENTITY_HW = (9, 12, 25, 49, 100)


def is_pow2(n):
    return n >= 1 and (n & (n - 1)) == 0


def inv_hw(HW):
    """1.0f / (float)HW: one correctly rounded fp32 division."""
    return torch.tensor(1.0, dtype=F32) / torch.tensor(float(HW), dtype=F32)


def acc_eps(S, n):
    return 2.0 * n * 2.0 ** -24 * S


class Operands(NamedTuple):
    x: torch.Tensor              # [B][HW][C] bf16
    w: torch.Tensor              # [N][C] fp32
    bias: torch.Tensor           # [N] fp32
    g: torch.Tensor              # [B][N] fp32
    k: Optional[torch.Tensor]    # exact leg, HW no power of two: the integer mean [B][C]


def operands(name, leg, B, HW, C, N):
    """leg 'exact' or 'gaussian'.  On the CPU; the GPU tests copy the very same tensors."""
    gen = rng(name, leg)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).double()
    k = None
    if leg == "exact":
        if is_pow2(HW):
            x = ri(-4, 4, B, HW, C) if HW < 64 else ri(-1, 4, B, HW, C)      # off centre: S grows past 8 bits
        else:
            k = ri(-2, 2, B, C)
            e = ri(-2, 2, B, HW // 2, C)
            d = torch.zeros(B, HW, C, dtype=F64)
            d[:, 0:2 * (HW // 2):2] = e
            d[:, 1:2 * (HW // 2):2] = -e
            d = d[:, torch.randperm(HW, generator=gen)]                 # the zero of an odd HW and the pairs land anywhere
            x = k[:, None, :] + d
        w, bias, g = ri(-4, 4, N, C), ri(-4, 4, N), ri(-4, 4, B, N)
    else:
        rn = lambda *shape: torch.randn(shape, generator=gen)
        x, w, bias, g = rn(B, HW, C), rn(N, C), rn(N), rn(B, N)
    return Operands(x.to(BF16).contiguous(), w.to(F32).contiguous(), bias.to(F32).contiguous(), g.to(F32).contiguous(), k)


# ------------------------------------------------------------------------------------------------------------ operations
def pool_sum(ar, x):
    """S [B][C] and sum |x| (reference only).  Emulation: fp32, pixel row r = hw % 8 summed in order, then r = 0 .. 7."""
    if "drop_last" in ar.mut:                                           # mutant: the last pixel is not summed
        x = x[:, :-1]
    xd = x.to(ar.dtype)
    if ar.ref:
        return xd.sum(1), xd.abs().sum(1)
    B, HW, C = x.shape
    rows = []
    for r in range(min(POOL_ROWS, max(HW, 1))):
        acc = torch.zeros(B, C, dtype=ar.dtype, device=x.device)
        for hw in range(r, HW, POOL_ROWS):
            acc = acc + xd[:, hw]
        rows.append(acc)
    s = torch.zeros(B, C, dtype=ar.dtype, device=x.device)
    for acc in rows:
        s = s + acc
    return s, None


def scale_f32(v, HW, ar=None):
    """f32(f32(v) * inv_hw): the ONE fp32 multiply of both passes, bit exact.  Over `Unrounded` alone: the real v / HW."""
    if isinstance(ar, Unrounded):
        return v.double() / HW
    return v.float() * inv_hw(HW).to(v.device)


def pooled_of(ar, S, HW):
    p = scale_f32(S, HW, ar)
    if "pooled_bf16" in ar.mut:                                         # mutant: the pooled features are rounded to bf16
        p = bf16_rne(p)
    return p


def logits_of(ar, pooled, w, bias):
    """bias + pooled @ w^T from the fp32 values handed in.  Returns (value in the arithmetic's dtype, sum |terms|)."""
    wd = w.to(ar.dtype)
    if "w_transposed" in ar.mut:                                        # mutant: the [N][C] storage is read as [C][N]
        wd = wd.reshape(wd.shape[1], wd.shape[0]).t()
    acc = ar.mm(pooled.to(ar.dtype), wd.t())
    if "no_bias" not in ar.mut:                                         # mutant: the bias is left out
        acc = acc + bias.to(ar.dtype)
    S = pooled.to(ar.dtype).abs() @ wd.abs().t() + bias.to(ar.dtype).abs() if ar.ref else None
    return acc, S


def gpooled_of(ar, g, w):
    acc = ar.mm(g.to(ar.dtype), w.to(ar.dtype))
    S = g.to(ar.dtype).abs() @ w.to(ar.dtype).abs() if ar.ref else None
    return acc, S


def gx_of(ar, gpooled, HW):
    """[B][HW][C] bf16 values from the STORED fp32 gpooled: one fp32 multiply, one rounding (`ar.rnd`: the `trunc` mutant)."""
    v = ar.rnd(scale_f32(gpooled, HW, ar))
    v = v if isinstance(ar, Unrounded) else v.bfloat16()
    return v[:, None, :].expand(v.shape[0], HW, v.shape[1]).contiguous()


class Results(NamedTuple):
    pooled: torch.Tensor         # fp32 [B][C]
    logits: torch.Tensor         # fp32 [B][N]
    gpooled: torch.Tensor        # fp32 [B][C]
    gx: torch.Tensor             # bf16 [B][HW][C]


def emulate(op, mut=()):
    """The fp32 emulation of both kernels (with mutants)."""
    ar = Arith(F32, GEMM_K, mut)
    HW = op.x.shape[1]
    S, _ = pool_sum(ar, op.x)
    pooled = pooled_of(ar, S, HW)
    logits, _ = logits_of(ar, pooled, op.w, op.bias)
    gp, _ = gpooled_of(ar, op.g, op.w)
    return Results(pooled.float(), logits.float(), gp.float(), gx_of(ar, gp.float(), HW))


# ------------------------------------------------------------------------------------------------------------ comparators
def assert_pool_identity(name, HW, k):
    """The premise of the exact leg for an HW that is no power of two: f32(f32(HW k) * f32(1 / HW)) == k, on the
    reference alone (k: any tensor of values with HW k exact in fp32)."""
    s = (k.double() * HW).float()
    assert bool((s.double() == k.double() * HW).all()), f"{name}: HW k is not exact in fp32"
    got = scale_f32(s, HW)
    bad = got.double() != k.double()
    assert not bool(bad.any()), f"{name}: f32(f32({HW} k) * f32(1/{HW})) != k for k = {float(k.reshape(-1)[bad.reshape(-1)][0])}"


def exact_references(name, B, HW, C, N):
    """Operands and the one correct value of each of the four outputs; every premise asserted on the reference alone."""
    op = operands(name, "exact", B, HW, C, N)
    ar = Arith()
    S, Sabs = pool_sum(ar, op.x)
    assert float(Sabs.max()) < 2.0 ** 23, f"{name}: sum |x| >= 2^23"
    assert bool((S == S.round()).all())
    if is_pow2(HW):
        q = 1.0 / HW
    else:
        q = 1.0
        assert torch.equal(S, op.k * HW), f"{name}: the deviations do not cancel"
        assert_pool_identity(name, HW, op.k)
    pooled = pooled_of(ar, S, HW)                                        # exact: S / HW resp. k
    assert bool((pooled.double() == S / HW).all()), f"{name}: pooled is not S / HW"
    logits, Sl = logits_of(ar, pooled, op.w, op.bias)
    assert float(Sl.max()) < 2.0 ** 23 * q, f"{name}: |pooled| @ |w| + |bias| = {float(Sl.max()) / q:.0f} quanta >= 2^23"
    assert bool((logits / q == (logits / q).round()).all()), f"{name}: the logits are no multiple of the quantum"
    gp, Sg = gpooled_of(ar, op.g, op.w)
    assert float(Sg.max()) < 2.0 ** 23, f"{name}: |g| @ |w| >= 2^23"
    assert bool((gp == gp.round()).all())
    gp32 = gp.float()
    print(name, "sum |terms| in quanta: pool %.0f logits %.0f gpooled %.0f; pooled values that are no bf16 values %.2f, gx "
          "values that are rounded %.2f" % (float(Sabs.max()), float(Sl.max()) / q, float(Sg.max()),
                                            float((bf16_rne(pooled) != pooled).double().mean()),
                                            float((bf16_rne(scale_f32(gp32, HW)) != scale_f32(gp32, HW)).double().mean())))
    return op, Results(pooled, logits.float(), gp32, gx_of(ar, gp32, HW))


def _bits(t):
    """int32 view of fp32 / int16 view of bf16, with -0.0 counted as +0."""
    t = t.detach().cpu().contiguous()
    t = torch.where(t == 0, torch.zeros_like(t), t)
    return t.view(torch.int16) if t.dtype == BF16 else t.float().view(torch.int32)


def compare_bits(name, got, want):
    """Raises on any bit that differs (a zero of either sign counts as zero)."""
    assert got.dtype == want.dtype, (name, got.dtype, want.dtype)
    got = got.reshape(want.shape)
    a, b = _bits(got), _bits(want)
    if torch.equal(a, b):
        return 0
    bad = a != b
    first = tuple(int(v) for v in bad.nonzero()[0])
    raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} outputs differ in bits; first at {first}: "
                         f"got {float(got[first])}, want {float(want[first])}")


def compare_exact(name, got, want):
    """got, want: Results.  All four outputs bit for bit."""
    for field in Results._fields:
        compare_bits(f"{name}/{field}", getattr(got, field), getattr(want, field))


def _ratio(got, r, bound):
    return float(((got.double().cpu().reshape(r.shape) - r).abs() / bound.clamp_min(2.0 ** -126)).max())


def gaussian_ratios(name, op, got):
    """max |got - r| / bound of pooled, logits (from got.pooled) and gpooled; gx bit for bit from got.gpooled.  Returns the
    three ratios."""
    ar = Arith()
    B, HW, C = op.x.shape
    u = 2.0 ** -24
    S, Sabs = pool_sum(ar, op.x)
    r, a = S / HW, acc_eps(Sabs, HW) / HW
    rp = _ratio(got.pooled, r, a + 2 * u * (r.abs() + a))
    rl_ref, Sl = logits_of(ar, got.pooled.cpu(), op.w, op.bias)
    rl = _ratio(got.logits, rl_ref, acc_eps(Sl, C + 1))
    rg_ref, Sg = gpooled_of(ar, op.g, op.w)
    rg = _ratio(got.gpooled, rg_ref, acc_eps(Sg, op.w.shape[0]))
    compare_bits(name + "/gx", got.gx, gx_of(ar, got.gpooled.cpu(), HW))
    return rp, rl, rg


def row_name(row, leg):
    return "head/%s/%s" % (tuple(row), leg)
