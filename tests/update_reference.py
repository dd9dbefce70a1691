"""Restatements, kernel emulations, operand generators and row checks for the parameter-update kernels of
csrc/adil_update.hip (AdamW, the l1 / l2 projections, ISTA, the atom constraints, the K x K inverse, the slab sum, the
fp8 copy and the evaluation sums).  numpy / torch CPU only: no GPU, no library.

Three layers:

restatements   the operation in float64 (or, for AdamW, in float32 with one rounding per operation, which is what the
               kernel computes: no contraction, IEEE division, correctly rounded square root);
emulations     numpy float32 in the kernel's own order (wave butterfly, rank sweep with the index tie-break, Michelot
               with fp64 sums, 32 slab accumulators and their tree, in-place Gauss-Jordan); each takes a `mutant` name
               and then computes the deliberately wrong variant the rows must reject;
checks         one function per row family.  It builds the seeded operands, calls `run` (the GPU wrapper in
               test_gpu_update_exact.py, an emulation in test_update_reference_cpu.py) and compares.  Both files go
               through the SAME function, so a row that the emulation passes is a row a correct kernel passes.

Two legs per family:

exact      operands on an integer grid chosen so that every intermediate of the kernel is exact up to the one or two
           roundings the model names: the bits must be EQUAL;
gaussian   N(0,1)-derived operands against float64, with the bound derived in the check's docstring; the worst
           err / bound is returned (and printed by the tests).
"""
import math

import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24                      # unit roundoff of fp32
TINY = float(np.finfo(np.float32).tiny)
Q = 2.0 ** -16                      # grid quantum of the l1 legs
R_GRID = 2.0 ** -5                  # radius of the exact l1 leg: 2048 quanta
R_GAUSS = 8 / 255                   # radius of the gaussian legs (the product's eps)
WAVE = 64


def _np(a):
    if torch.is_tensor(a):
        a = a.detach().cpu()
        if a.dtype == torch.bfloat16:
            a = a.float()
        a = a.numpy()
    return np.asarray(a)


# ============================================================================================================ comparators
def assert_bits_equal(got, want, what, ignore_zero_sign=False):
    """Same shape, same dtype, same bits.  ignore_zero_sign: True, or a boolean array naming the elements at which +0 and
    -0 count as equal."""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    if got.dtype == np.float32:
        gb, wb = got.view(np.uint32), want.view(np.uint32)
        bad = gb != wb
        if ignore_zero_sign is not False:
            both_zero = ((gb & 0x7fffffff) == 0) & ((wb & 0x7fffffff) == 0)
            bad &= ~(both_zero & np.broadcast_to(np.asarray(ignore_zero_sign, bool), bad.shape))
    else:
        bad = got != want
    if bad.any():
        i = np.unravel_index(int(np.argmax(bad)), bad.shape) if bad.ndim else ()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first at {i}: "
                             f"got {got[i]!r} want {want[i]!r}")


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound elementwise (float64); returns the worst err / bound (0 where both are 0)."""
    got, ref, bound = _np(got).astype(np.float64), _np(ref).astype(np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = np.abs(got - ref)
    bound = np.broadcast_to(bound, err.shape)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{what}: err / bound = {worst:.3f} at {i}: got {got[i]!r} ref {ref[i]!r} bound {bound[i]:.3e}")
    return worst


# ================================================================================================================== AdamW
def adamw_hyper(lr, t, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
    """(decay, b1, b2, eps, step_size, bc2_sqrt) of step t, formed in double as ops.AdamWSchedule forms them."""
    b1, b2 = betas
    return (1.0 - lr * weight_decay, b1, b2, eps, lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t))


def adamw_elem_f32(p, g, m, s, h, lo=None, hi=None, mutant=None):
    """adamw_elem of csrc/adil_common.h, then the clamp and max|q - p0| of adamw_clamp_kernel, in float32 with one
    rounding per operation.  The weights are 1.0f - b formed in fp32 (NOT torch's double 1 - beta rounded once).
    Returns (q, m, s, delta, smallest) with `smallest` the least non-zero magnitude among all intermediates: the rows
    assert it is a normal number, so the result does not depend on how subnormals are treated."""
    p, g, m, s = (np.asarray(a, F32) for a in (p, g, m, s))
    decay, b1, b2, eps, step, bc2 = (F32(v) for v in h)
    one = F32(1)
    w1, w2 = one - b1, one - b2
    if mutant == "torch_weights":
        w2 = F32(1.0 - float(h[2]))
    seen = []

    def k(x):
        nz = np.abs(x[x != 0])
        if nz.size:
            seen.append(float(nz.min()))
        return x

    with np.errstate(all="ignore"):
        pd = k(p * decay)
        m1 = k(m + k(w1 * k(g - m)))
        s1 = k(k(s * b2) + k(k(w2 * g) * g))
        if mutant == "eps_in_sqrt":
            den = k(np.sqrt(s1 + eps) / bc2)
        elif mutant == "no_bc2":
            den = k(np.sqrt(s1) + eps)
        else:
            den = k(k(k(np.sqrt(s1)) / bc2) + eps)
        upd = k(step * k(m1 / den))
        q = k((p - upd) * decay) if mutant == "decay_after" else k(pd - upd)
        pre = q
        if lo is not None:
            q = np.minimum(np.maximum(q, F32(lo)), F32(hi))
        dq = np.abs((pre if mutant == "delta_before_clamp" else q) - p)
    delta = F32(dq.max()) if dq.size else F32(0)
    return q.astype(F32), m1.astype(F32), s1.astype(F32), delta, (min(seen) if seen else 1.0)


def adamw_torch64(p, g, m, s, lr, t, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
    """torch.optim.AdamW, single tensor, in float64: (p, m, s) after step t."""
    b1, b2 = betas
    p, g, m, s = (np.asarray(a, np.float64) for a in (p, g, m, s))
    p = p * (1.0 - lr * weight_decay)
    m = m + (1.0 - b1) * (g - m)
    s = s * b2 + (1.0 - b2) * g * g
    denom = np.sqrt(s) / math.sqrt(1.0 - b2 ** t) + eps
    return p - (lr / (1.0 - b1 ** t)) * (m / denom), m, s


def emu_adamw_flat(p, g, m, s, h, lo, hi, mutant=None):
    """adamw_clamp_kernel: float4 body and the n % 4 tail run the same element function."""
    q, m1, s1, delta, small = adamw_elem_f32(p, _np(g), m, s, h, lo, hi, mutant)
    if mutant == "tail_skipped":
        n4 = (q.size // 4) * 4
        q[n4:], m1[n4:], s1[n4:] = p[n4:], m[n4:], s[n4:]
        delta = F32(np.abs(q - p).max())
    return dict(p=q, m=m1, s=s1, delta=delta, smallest=small)


# ============================================================================================================== slab sum
def slab_sum_exact(slabs):
    """Sum over the leading (slab) axis in int64: the operands of the slab rows are small integers."""
    s = np.asarray(slabs)
    assert np.array_equal(s, np.rint(s))
    return s.astype(np.int64).sum(axis=0)


def emu_slab_sum(slabs, nslabs, mutant=None):
    """slab_sum of adil_common.h: slab i goes to accumulator i % 32 in whole rounds of 32, the tail round reads clamped
    addresses and multiplies by 0/1 weights, the 32 accumulators meet in a pairwise tree.  slabs: (>= nslabs, ...)."""
    slabs = np.asarray(slabs, F32)
    acc = [np.zeros(slabs.shape[1:], F32) for _ in range(32)]
    s0 = 0
    with np.errstate(all="ignore"):
        while s0 + 32 <= nslabs:
            for u in range(32):
                acc[u] = acc[u] + slabs[s0 + u]
            s0 += 32
        if s0 < nslabs:
            for u in range(32):
                i = s0 + u
                w = F32(1.0) if (i < nslabs or mutant == "no_tail_weight") else F32(0.0)
                acc[u] = acc[u] + w * slabs[min(i, nslabs - 1)]
        w = 16
        while w >= 1:
            for u in range(w):
                acc[u] = acc[u] + acc[u + w]
            w //= 2
    return acc[0]


# =============================================================================================================== l1 ball
def l1ball_fp64(x, r, quantum=None):
    """Duchi's sort-based projection of every row of x (N, K) onto the l1 ball of radius r, in float64.  With `quantum`
    the operands are integers in units of it and everything up to the quotient is int64 arithmetic; `out` is then the
    kernel's rounding model in float32: theta32 = f32((c - r) / rho), the quotient formed in fp64 from exact operands (a
    correctly rounded fp32 division gives the same, 53 >= 2 * 24 + 2), then out = sign(x) max(f32(|x| - theta32), 0).
    Without it `out` is float64.  Rows with l1 norm < r (strict) come back untouched."""
    x = _np(x)
    x64 = x.astype(np.float64)
    n, kk = x64.shape
    if quantum is not None:
        xi = np.rint(x64 / quantum).astype(np.int64)
        ri = int(round(r / quantum))
        assert np.array_equal(xi * quantum, x64) and ri * quantum == r, "operands are not on the grid"
        a, rr, unit = np.abs(xi), ri, quantum
    else:
        a, rr, unit = np.abs(x64), float(r), 1.0
    big = a.sum(axis=1)
    mu = -np.sort(-a, axis=1)
    cs = np.cumsum(mu, axis=1)
    j = np.arange(1, kk + 1)
    rho = np.where(mu * j > cs - rr, j, 0).max(axis=1)
    safe = np.maximum(rho, 1)
    c = cs[np.arange(n), safe - 1]
    theta = ((c - rr) * unit) / safe                                   # one fp64 rounding on grid operands
    projected = ~(big < rr)
    tie = ((mu[:, 1:] == mu[:, :-1]) & (j[None, 1:] <= rho[:, None])).any(axis=1) if kk > 1 else np.zeros(n, bool)
    if quantum is not None:
        th32 = theta.astype(F32)
        pr = np.maximum(np.abs(x.astype(F32)) - th32[:, None], F32(0))
        out = np.where(projected[:, None], np.sign(x.astype(F32)) * pr, x.astype(F32)).astype(F32)
    else:
        pr = np.maximum(a - theta[:, None], 0.0)
        out = np.where(projected[:, None], np.sign(x64) * pr, x64)
    out[projected & (rho == 0)] = 0                                    # radius 0: theta is 0/0 and fmaxf(NaN, 0) = 0
    return dict(out=out, rho=rho, theta=np.where(projected, theta, 0.0), c=c * unit, S=big * unit,
                projected=projected, has_tie=tie & projected, on_boundary=(big == rr))


def _butterfly_sum(v):
    """wave_sum: xor-butterfly over the 64 lanes, fp32; every lane ends with the same value, lane 0 is returned."""
    v = v.astype(F32).copy()
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def emu_l1ball(x, r, mutant=None):
    """l1ball_row<EPL>: lane sums and butterfly for the l1 norm, descending rank and prefix of every element by one
    sequential sweep over the row (ties resolved by the index), rho = max rank that passes, theta, shrink."""
    x = np.asarray(x, F32)
    n, kk = x.shape
    epl = 1 if kk <= WAVE else 2
    w = WAVE * epl
    xs = np.zeros((n, w), F32)
    xs[:, :kk] = x
    a = np.abs(xs)
    r = F32(r)
    lane = a[:, :WAVE] if epl == 1 else a[:, :WAVE] + a[:, WAVE:]
    l1 = _butterfly_sum(lane)
    rank = np.ones((n, w), np.int32)
    pre = a.copy()
    idx = np.arange(w)
    for jj in range(w):
        aj = a[:, jj:jj + 1]
        before = aj > a
        if mutant != "no_tiebreak":
            before |= (aj == a) & (jj < idx)[None, :]
        rank += before
        pre = np.where(before, pre + aj, pre).astype(F32)
    cond = (a * rank.astype(F32)) > (pre - r)
    if mutant == "rho_min":
        rho = np.where(cond, rank, 1 << 20).min(axis=1)
    else:
        rho = np.where(cond, rank, 0).max(axis=1)
    cl = np.where(rank == rho[:, None], pre, F32(0)).astype(F32)
    c = _butterfly_sum(cl[:, :WAVE] if epl == 1 else cl[:, :WAVE] + cl[:, WAVE:])
    with np.errstate(all="ignore"):
        theta = (c - r) / (F32(kk) if mutant == "theta_over_k" else rho.astype(F32))
        pr = np.fmax(a - theta[:, None], F32(0))
    out = np.where(xs > 0, pr, np.where(xs < 0, -pr, F32(0) * pr)).astype(F32)
    if mutant == "sign_lost":
        out = pr.astype(F32)
    out = np.where((l1 < r)[:, None], xs, out)
    return out[:, :kk]


def emu_adamw_rows(v, g, m, s, h, radius, mutant=None):
    """adamw_l1ball_kernel on dense per-row gradients (zero rows outside the batch): AdamW, the projection when
    radius >= 0, max|v_new - v_old|."""
    q, m1, s1, _, small = adamw_elem_f32(v, g, m, s, h, mutant=mutant)
    if radius >= 0:
        q = emu_l1ball(q, radius, mutant)
    return dict(v=q, m=m1, s=s1, delta=F32(np.abs(q - np.asarray(v, F32)).max()), smallest=small)


def l1_grid_rows(kk, n, seed):
    """Integer-grid rows (quantum Q, radius R_GRID = 2048 quanta).  Amplitude 600 quanta for K >= 10 (about 0.8 of the rows
    project); for K < 10 it grows as 3 r / K so that more than half still do.  Every fifth row is heavy in ties, every
    seventh is small.  At n >= 16 rows 0..5 are: all zeros | l1 norm exactly r | one non-zero | rho = 1 beside small
    entries | all |x| = r (rho = K, theta = r (K-1)/K needs a rounding) | inside the ball."""
    rng = np.random.default_rng(1000 * kk + n + seed)
    ri = int(R_GRID / Q)
    amp = 600 if kk >= 10 else (3 * ri) // kk
    xi = rng.integers(-amp, amp + 1, size=(n, kk))
    if n >= 3:
        xi[::5] = rng.integers(-3, 4, size=xi[::5].shape) * (amp // 4)
        xi[::7] = rng.integers(-20, 21, size=xi[::7].shape)
    if n >= 16:
        xi[0] = 0
        xi[1] = 0
        if kk >= 2:
            xi[1, 0], xi[1, kk - 1] = ri // 2, -(ri // 2)
        else:
            xi[1, 0] = -ri
        xi[2] = 0
        xi[2, kk // 2] = -3 * ri
        xi[3] = rng.choice([-1, 1], size=kk)
        xi[3, kk - 1] = 4 * ri
        xi[4] = ri * rng.choice([-1, 1], size=kk)
        xi[5] = (ri // (2 * kk)) * rng.choice([-1, 1], size=kk)
    elif n == 3:
        xi[1] = 0
    return (xi * Q).astype(F32)


def l1_gauss_rows(kk, scale, seed, n=300):
    """N(0, scale^2) rows; every ninth row is zero in its upper half, rows 1, 5, 9, ... are rescaled to l1 norm ~ r."""
    rng = np.random.default_rng(seed)
    r = R_GAUSS
    x = (rng.standard_normal((n, kk)) * scale).astype(F32)
    x[::9, kk // 2:] = 0
    sm = np.abs(x[1::4].astype(np.float64)).sum(axis=1, keepdims=True)
    sm[sm == 0] = r
    x[1::4] = (x[1::4] * (r / sm)).astype(F32)
    return x


L1_K = (1, 2, 3, 10, 50, 63, 64, 65, 100, 127, 128)
L1_N = (1, 3, 257)
L1_GAUSS_K = (1, 2, 3, 10, 50, 64, 65, 100, 128)
IDENTITY_H = (1.0, 0.9, 0.999, 1e-8, 0.01, 1.0)     # with g = m = s = 0 adamw_elem returns p: p*1 - step*(0/eps)


def check_l1_exact(kk, run, seed=0):
    """run(x, r, fused) -> (out, delta or None).  fused = the AdamW + projection kernel with a zero gradient and
    IDENTITY_H, else l1ball_project_.  Bits equal the fp64 model; the sign of zero only where x != 0."""
    for n in L1_N:
        x = l1_grid_rows(kk, n, seed)
        ref = l1ball_fp64(x, R_GRID, Q)
        for fused in (False, True):
            out, delta = run(x.copy(), R_GRID, fused)
            assert_bits_equal(out, ref["out"], f"l1 exact K={kk} N={n} fused={fused}", ignore_zero_sign=(x == 0))
            if delta is not None:
                assert_bits_equal(F32(delta), F32(np.abs(ref["out"] - x).max()), f"l1 exact delta K={kk} N={n}")
    # radius 0: rho = 0, theta = 0/0, fmaxf(NaN, 0) = 0: every entry becomes a zero of either sign
    x = l1_grid_rows(kk, 3, seed + 1)
    out, _ = run(x.copy(), 0.0, False)
    assert_bits_equal(out, np.zeros_like(x), f"l1 radius 0 K={kk}", ignore_zero_sign=True)


def l1_gauss_scales(kk):
    return (0.003, 0.03, 1.0, 1.25 * R_GAUSS / kk)


def check_l1_gauss(kk, run):
    """|out - ref| <= u |ref| + 2 u (S + 2 theta), u = 2^-24, S the row's l1 norm, theta the reference threshold (0 for
    rows inside the ball).  theta's error is at most u (c + 2 theta): the sequential prefix c of positive terms, then the
    subtraction and the division; c <= S.  The factor 2 covers a row whose rho flips (theta is continuous across the
    flip) and a row whose fp32 norm falls on the other side of r (its theta is then of the order of u S).  The final
    subtraction adds u |ref|."""
    worst = 0.0
    for si, scale in enumerate(l1_gauss_scales(kk)):
        x = l1_gauss_rows(kk, scale, 100 * kk + si)
        ref = l1ball_fp64(x, R_GAUSS)
        out, _ = run(x.copy(), R_GAUSS, False)
        bound = U * np.abs(ref["out"]) + (2 * U * (ref["S"] + 2 * ref["theta"]))[:, None]
        worst = max(worst, assert_within(out, ref["out"], bound, f"l1 gauss K={kk} scale={scale:g}"))
    return worst


# ============================================================================================ strided atom rows (C,H,W,K)
def atom_l1ball_fp64(d, r, quantum=None):
    """l1ball_fp64 over the (channel, atom) rows of H*W pixels of a (C,H,W,K) tensor; with `quantum` the kernel's model:
    the fp64 threshold rounded to fp32 once (atom_l1ball_kernel), then the fp32 shrink."""
    d = _np(d)
    c, hh, ww, kk = d.shape
    rows = np.ascontiguousarray(d.reshape(c, hh * ww, kk).transpose(0, 2, 1)).reshape(c * kk, hh * ww)
    res = l1ball_fp64(rows, r, quantum)
    out = res["out"].reshape(c, kk, hh * ww).transpose(0, 2, 1).reshape(d.shape)
    return dict(res, out=np.ascontiguousarray(out))


def emu_atom_l1(d, r, mutant=None):
    """atom_l1ball_kernel: Michelot's iteration with fp64 sums (on grid operands every summation order gives the same
    sum, so the block tree is not restated), threshold rounded fp64 -> fp32 once, fp32 shrink."""
    d = np.asarray(d, F32)
    c, hh, ww, kk = d.shape
    out = d.reshape(c, hh * ww, kk).copy()
    r32 = F32(r)
    for ci in range(c):
        for k in range(kk):
            x = out[ci, :, k]
            a = np.abs(x).astype(np.float64)
            l1, cnt = a.sum(), float(a.size)
            if F32(l1) < r32:
                continue
            theta = (l1 - float(r32)) / cnt
            for _ in range(4096):
                act = (a >= theta) if mutant == "michelot_ge" else (a > theta)
                sm, nn = a[act].sum(), float(act.sum())
                if nn == cnt:
                    break
                cnt = nn
                with np.errstate(all="ignore"):
                    theta = (sm - float(r32)) / nn
            th = F32(theta)
            with np.errstate(all="ignore"):
                pr = np.fmax(np.abs(x) - th, F32(0))
            out[ci, :, k] = np.where(x > 0, pr, np.where(x < 0, -pr, F32(0) * pr)) if mutant != "sign_lost" else pr
    return out.reshape(d.shape)


ATOM_L1_SHAPES = ((1, 1, 1, 1), (3, 1, 5, 2), (3, 33, 31, 4), (3, 25, 41, 7), (2, 64, 64, 3))   # HW = 1, 5, 1023, 1025, 4096


def atom_l1_grid(shape, seed=0):
    """Grid dictionary (quantum Q, radius 1 = 65536 quanta), amplitude 3 r / HW so that most rows project, multiples of a
    coarse step so that ties abound.  With six rows or more: row (0,0) inside the ball, row (0,1) l1 norm exactly r, row
    (1,0) one entry above r beside unit entries (all but one drop)."""
    c, hh, ww, kk = shape
    hw = hh * ww
    rng = np.random.default_rng(7 * hw + kk + seed)
    ri = int(1.0 / Q)
    amp = max(8, (3 * ri) // hw)
    step = max(1, amp // 8)
    xi = rng.integers(-8, 9, size=(c, hw, kk)) * step
    if c * kk >= 6:
        xi[0, :, 0] = rng.choice([-1, 1], size=hw) * max(1, ri // (2 * hw))
        xi[0, :, 1] = 0
        xi[0, 0, 1], xi[0, hw - 1, 1] = ri // 2, -(ri - ri // 2)
        xi[1, :, 0] = rng.choice([-1, 0, 1], size=hw)
        xi[1, hw // 2, 0] = -2 * ri
    return (xi * Q).astype(F32).reshape(shape)


def check_atom_l1_exact(shape, run):
    """run(d, r) -> out.  Bits equal the model; the sign of zero only where d != 0."""
    d = atom_l1_grid(shape)
    ref = atom_l1ball_fp64(d, 1.0, Q)
    assert_bits_equal(run(d.copy(), 1.0), ref["out"], f"atom l1 {shape}", ignore_zero_sign=(d == 0))
    return ref


# =============================================================================================================== l2 ball
def l2ball_fp64(x, r):
    x = _np(x).astype(np.float64)
    nrm = np.sqrt((x * x).sum(axis=1, keepdims=True))
    return r * x / np.maximum(nrm, r)


def l2ball_model(x, r):
    """On integer rows (sum of squares exact): f32(f32(r x) / max(f32(sqrt(ss)), r))."""
    x = np.asarray(x, F32)
    ss = (x.astype(np.int64) ** 2).sum(axis=1, keepdims=True)
    assert ss.max() < 2 ** 24 and np.array_equal(x, np.rint(x))
    den = np.maximum(np.sqrt(ss.astype(np.float64)).astype(F32), F32(r))
    return ((F32(r) * x) / den).astype(F32)


def emu_l2ball(x, r, mutant=None):
    """l2ball_kernel<EPL>: per-lane sums of squares, butterfly, sqrt, max with r, (r x) / den."""
    x = np.asarray(x, F32)
    n, kk = x.shape
    epl = 1 if kk <= WAVE else 2
    xs = np.zeros((n, WAVE * epl), F32)
    xs[:, :kk] = x
    sq = xs * xs
    ss = _butterfly_sum(sq[:, :WAVE] if epl == 1 else sq[:, :WAVE] + sq[:, WAVE:])
    den = np.maximum(np.sqrt(ss), F32(r))[:, None]
    if mutant == "row_tail_skipped":
        out = x.copy()
        n4 = (n // 4) * 4
        out[:n4] = (F32(r) * x[:n4]) / den[:n4]
        return out
    return ((F32(r) * x) / den).astype(F32)


L2_K = (1, 3, 64, 65, 128)
L2_N = (1, 5, 258)
L2_R = 5.0


def l2_grid_rows(kk, n, seed=0):
    """Integer rows: dense ones outside the ball of radius 5, every third with at most three entries of magnitude <= 2
    (norm <= sqrt(12) < 5: inside), every fourth zero."""
    rng = np.random.default_rng(31 * kk + n + seed)
    amp = 9 if kk <= 3 else 3
    x = rng.integers(-amp, amp + 1, size=(n, kk))
    for i in range(0, n, 3):
        row = np.zeros(kk, np.int64)
        row[rng.integers(0, kk, size=3)] = rng.integers(-2, 3, size=3)
        x[i] = row
    x[3::4] = 0
    return x.astype(F32)


def check_l2_exact(kk, run):
    for n in L2_N:
        x = l2_grid_rows(kk, n)
        assert_bits_equal(run(x.copy(), L2_R), l2ball_model(x, L2_R), f"l2 exact K={kk} N={n}", ignore_zero_sign=(x == 0))


def check_l2_gauss(kk, run):
    """|out - ref| <= 3 u |ref| + u r.  The element path rounds three times (r x, the square root behind den, the
    division): 3 u |ref|.  What is left is the error of the sum of squares, (1 + EPL - 1 + 6) u at the most through the
    lane sum and the six butterfly levels, halved by the square root; it moves a whole row by the same factor.  For the
    rows of this leg (gaussian, K >= 3: |ref_i| well below r; K = 1: no addition at all) that is below u r, and rows
    inside the ball have den = r exactly."""
    worst = 0.0
    for si, scale in enumerate((0.003, 0.03, 1.0)):
        rng = np.random.default_rng(17 * kk + si)
        x = (rng.standard_normal((258, kk)) * scale).astype(F32)
        x[::9] *= F32(0.01)
        ref = l2ball_fp64(x, R_GAUSS)
        out = run(x.copy(), R_GAUSS)
        worst = max(worst, assert_within(out, ref, 3 * U * np.abs(ref) + U * R_GAUSS, f"l2 gauss K={kk} scale={scale:g}"))
    return worst


# ================================================================================================= atom norms and scaling
def atom_norms_fp64(d):
    d = _np(d).astype(np.float64)
    return np.sqrt((d.reshape(-1, d.shape[-1]) ** 2).sum(axis=0))


def atom_scale_fp64(d, sphere, radius=1.0):
    """constraint_dict 'l2sphere' / 'l2ball' for radius 1; otherwise the ball / sphere of that radius:
    d / max(|d| / r, 1) = r d / max(|d|, r)."""
    d = _np(d).astype(np.float64)
    n = atom_norms_fp64(d) / radius
    return d / (n if sphere else np.maximum(n, 1.0))


def atom_model(d, sphere, radius=1.0, unit=1.0):
    """On grid dictionaries (entries integer multiples of `unit`, a power of two, integer sum of squares < 2^24): norms =
    f32(sqrt(sum)), divided by the radius in fp32 when radius != 1 (ops.atom_l2_project_), d_out = f32(d / n) or
    f32(d / max(n, 1))."""
    d = np.asarray(d, F32)
    di = np.rint(d.astype(np.float64) / unit).astype(np.int64)
    assert np.array_equal(di * unit, d.astype(np.float64))
    ss = (di.reshape(-1, d.shape[-1]) ** 2).sum(axis=0)
    assert ss.max() < 2 ** 24
    norms = np.sqrt(ss.astype(np.float64) * unit * unit).astype(F32)
    n = norms if radius == 1.0 else (norms / F32(radius)).astype(F32)
    with np.errstate(all="ignore"):
        out = (d / (n if sphere else np.maximum(n, F32(1)))).astype(F32)
    return norms, out


def emu_atom_norms(d):
    """atom_sumsq_partial_kernel + atom_norm_finish_kernel in their order: thread (r, k) of a block walks its rows with
    stride R = 256 / KT, row 0 adds the R partials in order, the finish adds the blocks in order.  Products and sums are
    rounded separately here; the kernel may contract them (exact legs cannot tell, the gaussian bound admits both)."""
    d = np.asarray(d, F32)
    d2 = d.reshape(-1, d.shape[-1])
    p, kk = d2.shape
    rpb = (p + 511) // 512
    nb = (p + rpb - 1) // rpb
    kt = 16
    while kt < kk:
        kt *= 2
    rr = 256 // kt
    sq = np.zeros((nb * rpb, kk), F32)
    sq[:p] = d2 * d2
    sq = sq.reshape(nb, rpb, kk)
    part = None
    for r0 in range(rr):
        acc = np.zeros((nb, kk), F32)
        for i in range(r0, rpb, rr):
            acc = acc + sq[:, i]
        part = acc if part is None else part + acc
    tot = np.zeros(kk, F32)
    for b in range(nb):
        tot = tot + part[b]
    return np.sqrt(tot).astype(F32)


def emu_atom_project(d, sphere, radius=1.0, mutant=None):
    d = np.asarray(d, F32)
    norms = emu_atom_norms(d)
    n = norms if radius == 1.0 else (norms / F32(radius)).astype(F32)
    with np.errstate(all="ignore"):
        den = n if (sphere and mutant != "max_in_sphere") else np.maximum(n, F32(1))
        return norms, (d / den).astype(F32)


ATOM_SHAPES = ((1, 1), (7, 3), (300, 17), (512, 33), (513, 65), (1031, 100), (2048, 128))
ATOM_UNIT = 2.0 ** -3


def atom_grid(p, kk, seed=0):
    """Entries in {-3..3} / 8.  Atom 0 has at most two non-zero rows (norm < 1: the ball leaves it, the sphere stretches
    it), every other atom with P >= 8 has norm > 1.  No atom is zero (the sphere would divide by 0)."""
    rng = np.random.default_rng(13 * p + kk + seed)
    di = rng.integers(-3, 4, size=(p, kk))
    di[0] = rng.choice([-3, -2, -1, 1, 2, 3], size=kk)
    di[2:, 0] = 0
    return (di * ATOM_UNIT).astype(F32)


def check_atom_exact(p, kk, run):
    """run(d, sphere, radius) -> (norms, d_out) with norms as ops.atom_norms gives them (before the radius)."""
    d = atom_grid(p, kk)
    for sphere, radius in ((False, 1.0), (True, 1.0), (False, 0.5), (True, 0.5)):
        norms, out = run(d.copy(), sphere, radius)
        wn, wo = atom_model(d, sphere, radius, ATOM_UNIT)
        assert_bits_equal(norms, wn, f"atom norms P={p} K={kk}")
        assert_bits_equal(out, wo, f"atom scale P={p} K={kk} sphere={sphere} radius={radius}", ignore_zero_sign=(d == 0))


ATOM_GAUSS = (3 * 64 * 64, 50)


def check_atom_gauss(run):
    """Relative bound u (P/512 + 9 + 2) on the norms and on the scaled dictionary: P/512 additions per thread, log2(512) =
    9 for the two later stages (the R partials of a block and the 512 block sums; the finish adds them one after the
    other, so this is the depth a tree would have: the bound leans on the errors being rounding noise, not all of one
    sign), 2 for the square root and the division."""
    p, kk = ATOM_GAUSS
    rng = np.random.default_rng(5)
    d = rng.standard_normal((p, kk)).astype(F32) * F32(0.02)
    d[:, 0] *= F32(0.1)                                            # atom 0 inside the unit ball
    rel = U * (p / 512 + 9 + 2)
    worst = 0.0
    for sphere in (False, True):
        norms, out = run(d.copy(), sphere, 1.0)
        worst = max(worst, assert_within(norms, atom_norms_fp64(d), rel * atom_norms_fp64(d), "atom norms gauss"))
        ref = atom_scale_fp64(d, sphere)
        worst = max(worst, assert_within(out, ref, rel * np.abs(ref), f"atom scale gauss sphere={sphere}"))
    return worst


# ================================================================================================================== ISTA
def ista_fp64(v, g, step, lam):
    t = _np(v).astype(np.float64)
    if g is not None:
        t = t - step * _np(g).astype(np.float64)
    return np.where(t > lam, t - lam, np.where(t < -lam, t + lam, 0.0))


def emu_ista(v, g, step, lam, mutant=None):
    t = np.asarray(v, F32)
    if g is not None:
        t = t - F32(step) * np.asarray(g, F32)
    lam = F32(lam)
    if mutant == "sign_lost":
        return np.where(np.abs(t) > lam, np.abs(t) - lam, F32(0)).astype(F32)
    return np.where(t > lam, t - lam, np.where(t < -lam, t + lam, F32(0))).astype(F32)


ISTA_N = (2048 * 256 + 5, 37 * 50)


def check_ista_exact(n, run):
    """Grid v, g (multiples of 2^-10, |.| <= 1), step 2^-2, lam 2^-3: t and the shrink are exact, fused or not; values
    with |t| == lam (strict comparisons) are frequent.  Bits equal, zero sign included (the kernel writes +0)."""
    rng = np.random.default_rng(n)
    v = (rng.integers(-1024, 1025, size=n) * 2.0 ** -10).astype(F32)
    g = (rng.integers(-1024, 1025, size=n) * 2.0 ** -10).astype(F32)
    v[::11] = F32(0.125)
    v[5::11] = F32(-0.125)
    g[::22] = 0
    for gg in (g, None):
        want = ista_fp64(v, gg, 0.25, 0.125).astype(F32)
        assert_bits_equal(run(v.copy(), gg, 0.25, 0.125), want, f"ista exact n={n} g={'yes' if gg is not None else 'None'}")


def check_ista_gauss(n, run):
    """|out - ref| <= u (|t| + |step g| + |out|): the product, the subtraction and the shrink round once each; a fused
    t - step g drops the first term, so both forms are inside."""
    rng = np.random.default_rng(n + 1)
    v = (rng.standard_normal(n) * 0.05).astype(F32)
    g = rng.standard_normal(n).astype(F32)
    step, lam = 0.013, 0.02
    s32, l32 = float(F32(step)), float(F32(lam))                   # the kernel receives the scalars as fp32
    ref = ista_fp64(v, g, s32, l32)
    t = v.astype(np.float64) - s32 * g.astype(np.float64)
    bound = U * (np.abs(t) + np.abs(s32 * g.astype(np.float64)) + np.abs(ref))
    # an element whose t lies within the bound of +-lam may fall on either side of the comparison: the shrink is
    # continuous there, so the same bound holds
    return assert_within(run(v.copy(), g, step, lam), ref, bound, f"ista gauss n={n}")


# ========================================================================================================= the SPD family
def spd_family(kk, seed=0):
    """A = L L^T with L unit lower bidiagonal, sub-diagonal +-1: A and A^-1 are integer matrices (|A| <= 2,
    |A^-1| <= K, no zero in A^-1) and every Gauss-Jordan pivot is 1.  Returns (A fp32, A^-1 float64)."""
    rng = np.random.default_rng(kk + 977 * seed)
    lo = np.eye(kk)
    for i in range(kk - 1):
        lo[i + 1, i] = rng.choice([-1.0, 1.0])
    a = lo @ lo.T
    li = np.rint(np.linalg.inv(lo))
    inv = li.T @ li
    assert np.array_equal(a @ inv, np.eye(kk))
    return a.astype(F32), inv


def emu_spd_inverse(a, mutant=None):
    """spd_inverse_kernel: in-place Gauss-Jordan without pivoting in fp64, the hardware reciprocal and its two Newton
    steps replaced by an exact reciprocal (pivots are 1 in the family), result rounded to fp32."""
    t = np.asarray(a, np.float64).copy()
    kk = t.shape[0]
    for k in range(kk):
        piv = 1.0 / t[k, k]
        row = t[k, :] * piv
        row[k] = piv
        col = t[:, k].copy()
        new = t.copy()
        new[:, k] = 0.0
        new = new - np.outer(col, row)
        new[k, :] = row
        if mutant == "pivot_column_kept" and k == kk - 1:
            new[:, k] = t[:, k]
        t = new
    return t.astype(F32)


SPD_K = tuple(range(1, 13)) + (16, 17, 63, 64, 65, 100, 127, 128)


def check_spd(kk, run):
    a, inv = spd_family(kk)
    assert_bits_equal(run(a.copy()), inv.astype(F32), f"spd_inverse K={kk}", ignore_zero_sign=True)


# ======================================================================================================== image metrics
def image_metrics_fp64(adv, x):
    a, b = _np(adv).astype(np.float64), _np(x).astype(np.float64)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    return ((a - b) ** 2).sum(axis=1), (b * b).sum(axis=1)


def emu_image_metrics(adv, x, mutant=None):
    """image_metrics_kernel on the exact leg: every partial sum is an integer multiple of 2^-8 below 2^16, so the fp32
    sums equal the integer sums in every order; the thread / wave / block order is not restated."""
    a, b = _np(adv).astype(F32), _np(x).astype(F32)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    if mutant == "vector_tail_dropped":
        p8 = (a.shape[1] // 8) * 8
        a, b = a[:, :p8], b[:, :p8]
    dv = a - b
    return (dv * dv).sum(axis=1, dtype=F32), (b * b).sum(axis=1, dtype=F32)


METRIC_P = (1, 7, 8, 63, 4096, 8200, 12288, 50000)


def metrics_operands(p, dtype, seed=0, batch=3):
    """adv, x in {0..16}/16 (exact in bf16 and fp32; squares are multiples of 2^-8, image sums stay below 2^24 / 256)."""
    g = torch.Generator().manual_seed(p + seed)
    adv = (torch.randint(0, 17, (batch, p), generator=g).float() / 16).to(dtype)
    x = (torch.randint(0, 17, (batch, p), generator=g).float() / 16).to(dtype)
    return adv, x


def check_metrics_exact(p, dtype, run):
    """run(adv, x, misalign) -> (sq_err, sq_norm).  misalign: x is handed over as a view one element off a 16-byte
    boundary, which sends a size that would take 16-byte loads down the element route."""
    adv, x = metrics_operands(p, dtype)
    we, wn = image_metrics_fp64(adv, x)
    for misalign in (False, True):
        se, sn = run(adv, x, misalign)
        assert_bits_equal(se, we.astype(F32), f"sq_err P={p} {dtype} misalign={misalign}")
        assert_bits_equal(sn, wn.astype(F32), f"sq_norm P={p} {dtype} misalign={misalign}")


# =================================================================================================================== fp8
def fp8_bytes(x, scale=256.0):
    """The fp8 operand encoding of a dictionary: e4m3(clamp(256 x, -448, 448)) as bytes (oracle.synth_fp8's quantiser)."""
    x = torch.as_tensor(_np(x).astype(np.float32))
    return (x * scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def fp8_probe_values():
    """Every finite e4m3 value / 256, the midpoint of every neighbouring pair (ties go to the even byte), and +-2.0
    (512 before the clamp: saturates at 448); padded with zeros to a multiple of 4."""
    vals = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    vals = torch.sort(vals[torch.isfinite(vals)]).values.double()
    mids = (vals[1:] + vals[:-1]) / 2
    x = (torch.cat([vals, mids, torch.tensor([2.0 * 256, -2.0 * 256], dtype=torch.float64)]) / 256).float().numpy()
    assert np.array_equal(x.astype(np.float64) * 256, torch.cat([vals, mids, torch.tensor([512.0, -512.0],
                                                                 dtype=torch.float64)]).numpy())
    return np.concatenate([x, np.zeros((-x.size) % 4, F32)])


def check_fp8(run):
    x = fp8_probe_values()
    assert_bits_equal(run(x.copy()), fp8_bytes(x), "dict_to_fp8 probe values")


# =========================================================================================== flat AdamW rows (adamw_clamp)
ADAMW_N = (1, 2, 3, 4, 5, 7, 1023, 1025, 4 * 2048 * 256 + 4 * 777 + 3)
ADAMW_FP8_N = (4, 1024, 4 * 2048 * 256 + 8)
ADAMW_CLAMPS = ((-0.5, 0.5), (0.25, 0.25))
BOGUS = (123.0, 0.5)                # host step_size / bc2_sqrt of the `dyn` row: must be ignored


def adamw_operands(n, gdtype, seed=0, steps=3):
    """p ~ N(0,1); g ~ N(0,1) with exact zeros on every third element, in the gradient dtype."""
    gen = torch.Generator().manual_seed(n * 3 + seed)
    p = torch.randn(n, generator=gen).numpy()
    gs = []
    for _ in range(steps):
        g = torch.randn(n, generator=gen)
        g[1::3] = 0.0
        gs.append(g.to(gdtype))
    return p, gs


def check_adamw_flat(n, gdtype, run, clamps=ADAMW_CLAMPS, dyn=False, fp8=False, lr=0.01):
    """run(p, g, m, s, h, lo, hi, dyn, fp8) -> dict(p, m, s, delta[, fp8]); h is what the host passes, dyn the two
    step-dependent scalars for the device buffer (or None).  Three consecutive steps per clamp range; p, m, s and
    max|delta| are compared after every step; no intermediate of the reference is subnormal."""
    for lo, hi in clamps:
        p, gs = adamw_operands(n, gdtype)
        m, s = np.zeros(n, F32), np.zeros(n, F32)
        for t, g in enumerate(gs, 1):
            h = adamw_hyper(lr, t)
            want = emu_adamw_flat(p, g, m, s, h, lo, hi)
            assert want["smallest"] >= TINY, ("subnormal intermediate in the reference", want["smallest"])
            host_h = h[:4] + BOGUS if dyn else h
            got = run(p.copy(), g, m.copy(), s.copy(), host_h, lo, hi, (h[4], h[5]) if dyn else None, fp8)
            what = f"adamw n={n} {gdtype} clamp=({lo},{hi}) step {t} dyn={dyn}"
            for key in ("p", "m", "s"):
                assert_bits_equal(got[key], want[key], f"{what}: {key}")
            assert_bits_equal(F32(got["delta"]), want["delta"], f"{what}: max_abs_delta")
            if fp8:
                assert_bits_equal(got["fp8"], fp8_bytes(want["p"]), f"{what}: p_fp8")
            p, m, s = want["p"], want["m"], want["s"]


# =================================================================================== AdamW on rows (adamw_l1ball, r < 0)
ROWS_NK = ((1, 1), (5, 3), (257, 50), (130, 64), (67, 65), (33, 128))
ROW_SOURCES = ("dense", "pos", "slab")


def rows_operands(n, kk, source, seed=0):
    """v ~ N(0, 0.1^2), m, s from one earlier step (non-zero state).  Returns the state, the gradient source as the
    wrapper needs it and the dense (N, K) gradient it stands for.
    dense: one gradient row per row of v | pos: batch rows {0, 1, N-1}, slot table otherwise -1 | slab: small-integer
    slabs (5 of them, plus one of NaN that must never be read) over the batch rows of `pos`."""
    rng = np.random.default_rng(97 * n + kk + seed)
    v = (rng.standard_normal((n, kk)) * 0.1).astype(F32)
    g0 = rng.standard_normal((n, kk)).astype(F32)
    _, m, s, _, _ = adamw_elem_f32(v, g0, np.zeros_like(v), np.zeros_like(v), adamw_hyper(0.01, 1))
    batch_rows = sorted({0, min(1, n - 1), n - 1})
    pos = np.full(n, -1, np.int32)
    spec = dict(kind=source)
    if source == "dense":
        g = rng.standard_normal((n, kk)).astype(F32)
        g[1::3] = 0
        spec.update(g=g)
    else:
        perm = rng.permutation(len(batch_rows))
        for slot, row in zip(perm, batch_rows):
            pos[row] = slot
        b = len(batch_rows)
        if source == "pos":
            gb = rng.standard_normal((b, kk)).astype(F32)
            spec.update(g=gb, pos=pos.copy())
        else:
            nslabs, rows = 5, b + 2
            slabs = rng.integers(-9, 10, size=(nslabs + 1, rows, kk)).astype(F32)
            slabs[nslabs] = np.nan
            gb = slab_sum_exact(slabs[:nslabs]).astype(F32)[:b]
            spec.update(slabs=slabs, nslabs=nslabs, rows=rows, batch=b, pos=pos.copy())
        g = np.zeros((n, kk), F32)
        for row in batch_rows:
            g[row] = gb[pos[row]]
    return v, m, s, spec, g


def check_adamw_rows(n, kk, source, run):
    """run(v, m, s, spec, h, radius) -> dict(v, m, s, delta, pos).  radius = -1: AdamW alone.  pos comes back all -1."""
    v, m, s, spec, g = rows_operands(n, kk, source)
    h = adamw_hyper(0.01, 2)
    want = emu_adamw_rows(v, g, m, s, h, -1.0)
    assert want["smallest"] >= TINY
    got = run(v.copy(), m.copy(), s.copy(), spec, h, -1.0)
    what = f"adamw rows N={n} K={kk} {source}"
    for key in ("v", "m", "s"):
        assert np.isfinite(_np(got[key])).all(), f"{what}: {key} not finite"
        assert_bits_equal(got[key], want[key], f"{what}: {key}")
    assert_bits_equal(F32(got["delta"]), want["delta"], f"{what}: max_abs_delta")
    if source != "dense":
        assert_bits_equal(got["pos"], np.full(n, -1, np.int32), f"{what}: pos")


# ============================================================================================================= slab rows
SLAB_COUNTS = (1, 2, 31, 32, 33, 63, 64, 65, 236)
SLAB_B, SLAB_K = 5, 50


def slab_operands(nslabs, seed=0):
    """(nslabs + 1, B + 1, K) small integers; the last slab is NaN: it sits where an unclamped tail address would read."""
    rng = np.random.default_rng(nslabs + seed)
    slabs = rng.integers(-50, 51, size=(nslabs + 1, SLAB_B + 1, SLAB_K)).astype(F32)
    slabs[nslabs] = np.nan
    return slabs


def check_slab(nslabs, run_pack, run_rows):
    """run_pack(slabs, nslabs, rows, batch, k) -> the padded code matrix of pack_codes; run_rows as in check_adamw_rows.
    The sums must equal the integer sums and nothing may be NaN (padding is zero)."""
    slabs = slab_operands(nslabs)
    want = slab_sum_exact(slabs[:nslabs])[:SLAB_B].astype(F32)
    vp = _np(run_pack(slabs, nslabs, SLAB_B + 1, SLAB_B, SLAB_K))
    assert np.isfinite(vp).all(), f"pack_codes nslabs={nslabs}: NaN / Inf"
    assert_bits_equal(vp[:SLAB_B, :SLAB_K], want, f"pack_codes nslabs={nslabs}", ignore_zero_sign=True)
    pad = vp.copy()
    pad[:SLAB_B, :SLAB_K] = 0
    assert not pad.any(), f"pack_codes nslabs={nslabs}: padding not zero"
    # through AdamW: no slot table, row b <-> slab row b
    rng = np.random.default_rng(nslabs + 1)
    v = (rng.standard_normal((SLAB_B, SLAB_K)) * 0.1).astype(F32)
    m, s = np.zeros_like(v), np.zeros_like(v)
    h = adamw_hyper(0.01, 1)
    spec = dict(kind="slab", slabs=slabs, nslabs=nslabs, rows=SLAB_B + 1, batch=SLAB_B, pos=None)
    got = run_rows(v.copy(), m, s, spec, h, -1.0)
    ref = emu_adamw_rows(v, want, m, s, h, -1.0)
    for key in ("v", "m", "s"):
        assert np.isfinite(_np(got[key])).all(), f"adamw slab nslabs={nslabs}: {key} not finite"
        assert_bits_equal(got[key], ref[key], f"adamw slab nslabs={nslabs}: {key}")
