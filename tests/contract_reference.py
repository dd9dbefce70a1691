"""Restatements, kernel emulations, operand generators and row checks for the contractions of csrc/adil_contract.hip:
the synthesis (adil_synth, adil_synth_store, adil_synth_fp8, adil_synth_fp8_packed) and the z-step (adil_zstep,
adil_zstep_codes).  numpy / torch CPU only: no GPU, no library.  The layout is that of update_reference.py.

restatements   the operation in float64, on the operands the kernel multiplies (bf16 streams: rne_bf16(D), rne_bf16(V);
               fp8: the e4m3 quantiser of update_reference.fp8_bytes with saturation at +-448; fp32 streams: exact);
emulations     numpy float32: fp32 streams split every operand three ways, h = rne(x), m = rne(x - h), l = rne(x - h - m),
               and issue the six piece products of Mma<float>::mma in the kernel's order per k-group of 16, each
               accumulated in fp32; bf16 and fp8 streams issue one product.  The tile order of the kernels is NOT
               followed: on the exact legs every partial sum is exact, so any order gives the same bits.  Each emulation
               takes a `mutant` name and then computes the deliberately wrong variant the rows must reject;
checks         one function per row family.  It builds the operands seeded from the row id, calls `run` (the wrapper
               around ops in test_gpu_contract_exact.py, an emulation in test_contract_reference_cpu.py) and compares.

Two legs:

exact      operands on one of four grids on which every product and every partial sum of the kernel is exact in fp32,
           up to the single rounding to the stream type at the store.  The premise is asserted on the reference alone,
           in float64: every operand is a multiple of its quantum and sum |terms| + |x| < 2^24 q for the row's product
           quantum q.  Then the bits must be EQUAL; only the sign of a zero is not compared; no element is excluded.
             narrow  <= 8 significant bits (bf16-exact, m = l = 0): D = i 2^-7 (|i| <= 127), V = j 2^-7 (|j| <= 7),
                     x in {0..128}/128, q = 2^-14.  x + V D^T needs more than 8 bits: the bf16 store rounds, ties occur.
             mid     9..16 significant bits (m plane non-zero, l = 0; hh, hm, mh, mm all contribute).  Nine-bit operands
                     are exactly halfway between two bf16 numbers: RNE and truncation of the operand differ.
             wide    one operand with 24 significant bits (h, m, l non-zero) against a partner +-2^e with one non-zero
                     term per output: the output is the 24-bit value shifted.  Both ways round.
             fp8     fp8_absmax = 0.75 2^n: every scale is a power of two; one set of codes is e4m3-exact after scaling,
                     a dense second set consists of ties of the conversion and a sparse third one saturates beyond 448:
                     the reference quantises both (fp8_dv, with the model of the fp8 MFMA's sum they rest on).
gaussian   D ~ U[-1, 1], V ~ 0.02 N(0,1), g ~ N(0,1), x ~ U[0, 1] against float64 with an elementwise bound derived in
           gauss_bound; the worst err / bound is returned (and printed by the tests).
"""
import zlib
from typing import NamedTuple, Optional

import numpy as np
import torch

import update_reference as U
from test_gpu_routes import ROUTES
from update_reference import F32, _np, assert_bits_equal, assert_within

U24 = 2.0 ** -24
SENTINEL = 4096.0                                # what surrounds every output (test_gpu_routes.SENTINEL)
KGROUP = 16
# the six piece products of Mma<float>::mma, (piece of a, piece of b), in issue order: small terms first
PRODUCTS = (("l", "h"), ("h", "l"), ("m", "m"), ("m", "h"), ("h", "m"), ("h", "h"))
DROP_MUTANTS = tuple(f"drop_{pa}{pb}" for pa, pb in PRODUCTS)


def seed_of(name):
    return zlib.crc32(name.encode())


def round_up(x, m):
    return (x + m - 1) // m * m


# ============================================================================================================ number formats
def rne_bf16(a):
    """float32 -> nearest bf16 (ties to even), returned as float32."""
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(torch.bfloat16).float().numpy()


def trunc_bf16(a):
    """float32 -> bf16 by dropping the low 16 bits (the wrong conversion: a mutant)."""
    return (np.ascontiguousarray(a, F32).view(np.uint32) & np.uint32(0xffff0000)).view(F32)


def split3(a, rnd=rne_bf16):
    """Mma<float>::split2: x = h + m + l, every piece a bf16 value; the subtractions are exact in fp32."""
    a = np.asarray(a, F32)
    h = rnd(a)
    r = (a - h).astype(F32)
    m = rnd(r)
    r = (r - m).astype(F32)
    return dict(h=h, m=m, l=rnd(r))


def e4m3(a, saturate=True):
    """float32 -> OCP e4m3 (ties to even) as float32; saturate: fp8_range first (the kernel always does)."""
    t = torch.from_numpy(np.ascontiguousarray(a, F32))
    if saturate:
        t = t.clamp(-448.0, 448.0)
    return t.to(torch.float8_e4m3fn).float().numpy()


def sig_bits(a):
    """Number of significant bits of every element of a float array (0 for 0): position of the top set bit minus the
    position of the lowest set bit of the 24-bit significand, plus one."""
    a = np.abs(np.asarray(a, np.float64))
    mant, _ = np.frexp(a)
    i = np.rint(mant * 2.0 ** 53).astype(np.int64)                    # exact for anything with <= 53 bits
    low = i & -i
    out = np.zeros(a.shape, np.int64)
    nz = i != 0
    out[nz] = 53 - np.log2(low[nz]).astype(np.int64)
    return out


# ============================================================================================================ the contraction
def emu_contract(a, b, stream, acc0=None, mutant=None, kgroup=KGROUP):
    """acc (M, N) float32 = acc0 + a (M, K) b (K, N) the way the MFMA loops form it.  K is zero-padded to a multiple of
    `kgroup` (16; 32 in the code contraction of zstep_codes_kernel).  Per k-group the piece products of the stream type
    are issued in order, each accumulated in fp32: the terms of one MFMA are summed in float64 and rounded once, which
    is exact on the exact legs and one admissible order on the gaussian leg.
    stream: "f32" (six products of the three-way split) | "bf16" (operands rounded to bf16, one product) |
            "raw" (operands used as they are, one product: fp8 operands, already quantised).
    mutants: drop_<pa><pb> one of the six products missing | swap_ml the m and l planes of b exchanged |
             trunc_operand bf16 conversion of the operands by truncation | skip_last_group | pad_not_zeroed (the
             padded reduction indices of b hold NaN bits instead of 0)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    mm, kk = a.shape
    nn = b.shape[1]
    kp = round_up(kk, kgroup)
    ap = np.zeros((mm, kp), F32)
    ap[:, :kk] = a
    bp = np.full((kp, nn), np.nan if mutant == "pad_not_zeroed" else 0.0, F32)
    bp[:kk] = b
    rnd = trunc_bf16 if mutant == "trunc_operand" else rne_bf16
    if stream == "f32":
        pa, pb = split3(ap, rnd), split3(bp, rnd)
        if mutant == "swap_ml":
            pb["m"], pb["l"] = pb["l"], pb["m"]
        prods = [(pa[x].astype(np.float64), pb[y].astype(np.float64)) for x, y in PRODUCTS if mutant != f"drop_{x}{y}"]
    elif stream == "bf16":
        prods = [(rnd(ap).astype(np.float64), rnd(bp).astype(np.float64))]
    else:
        prods = [(ap.astype(np.float64), bp.astype(np.float64))]
    acc = np.zeros((mm, nn), F32) if acc0 is None else np.array(acc0, F32, copy=True)
    ngroups = kp // kgroup - (1 if mutant == "skip_last_group" else 0)
    with np.errstate(all="ignore"):
        for g in range(ngroups):
            sl = slice(kgroup * g, kgroup * (g + 1))
            for x, y in prods:
                acc = (acc.astype(np.float64) + x[:, sl] @ y[sl]).astype(F32)
    return acc


def operands64(a, stream):
    """An operand as the kernel multiplies it, in float64."""
    a = np.asarray(a, F32)
    return (rne_bf16(a) if stream == "bf16" else a).astype(np.float64)


# ================================================================================================================ synthesis
class SynthCase(NamedTuple):
    """One call of the synthesis.  x (B, P) float32 holding stream-exact values, or None; d (P, K); v (B, K); stream the
    image stream type ("f32" | "bf16"); fp8 = fp8_absmax or None; packed: through dict_to_fp8 + adil_synth_fp8_packed;
    x_off / out_off: elements past a 16-byte boundary; q: product quantum of an exact case (None: gaussian)."""
    name: str
    x: Optional[np.ndarray]
    d: np.ndarray
    v: np.ndarray
    stream: str
    delta: float = -1.0
    pixel: bool = False
    fp8: Optional[float] = None
    packed: bool = False
    x_off: int = 0
    out_off: int = 0
    q: Optional[float] = None


def fp8_scales(absmax):
    """OpScale of fp8_scale(): code scale 384 / absmax, dictionary scale 256, output scale 1 / (v d), formed in fp32."""
    v = F32(384.0) / F32(absmax)
    d = F32(256.0)
    return v, d, F32(1.0) / F32(v * d)


def synth_operands64(c, saturate=True):
    """(V, D) of a case as the kernel multiplies them, in float64, in the units of the images."""
    if c.fp8 is None:
        return operands64(c.v, c.stream), operands64(c.d, c.stream)
    sv, sd, so = fp8_scales(c.fp8)
    qv = e4m3((np.asarray(c.v, F32) * sv).astype(F32), saturate).astype(np.float64)
    qd = e4m3((np.asarray(c.d, F32) * sd).astype(F32), saturate).astype(np.float64)
    return qv * float(so), qd                      # so = 1 / (sv sd) carries both scales: qv qd so is the product


def ref_synth(c):
    """out = clamp01?(x + clamp_delta?(V D^T)) in float64, NOT yet rounded to the stream type, and S = |V| |D|^T + |x|.
    delta is the float32 the kernel receives."""
    v, d = synth_operands64(c)
    dv = v @ d.T
    s = np.abs(v) @ np.abs(d).T
    if c.delta >= 0:
        dl = float(F32(c.delta))
        dv = np.clip(dv, -dl, dl)
    if c.x is not None:
        dv = dv + c.x.astype(np.float64)
        s = s + np.abs(c.x.astype(np.float64))
    if c.pixel:
        dv = np.clip(dv, 0.0, 1.0)
    return dv, s


def round_stream(r64, stream, what=""):
    """The one rounding of an exact row: the float64 result is an fp32 number (premise), the bf16 store rounds it."""
    r32 = r64.astype(F32)
    assert np.array_equal(r32.astype(np.float64), r64), f"{what}: the reference is not an fp32 number"
    return rne_bf16(r32) if stream == "bf16" else r32


def emu_synth(c, mutant=None):
    """synth_mfma_kernel: XACC (x present, delta_clamp < 0) loads x into the accumulators; otherwise the epilogue is
    clamp(acc, +-delta) + x; then the pixel clamp and one conversion to the stream type.  Returns dict(out, clean).
    mutants (beside emu_contract's): trunc_out | delta_after_x | pixel_before_delta | x_twice | row_ge_B_stored |
    fp8_scale_128 | fp8_no_saturation."""
    b, p = c.v.shape[0], c.d.shape[0]
    xacc = c.x is not None and c.delta < 0
    x = None if c.x is None else np.asarray(c.x, F32)
    cm = mutant if mutant in DROP_MUTANTS + ("swap_ml", "trunc_operand", "skip_last_group", "pad_not_zeroed") else None
    with np.errstate(all="ignore"):
        if c.fp8 is None:
            acc = emu_contract(c.v, c.d.T, c.stream, x if xacc else None, cm)
        else:
            sv, sd, so = fp8_scales(c.fp8)
            sat = mutant != "fp8_no_saturation"
            qv = e4m3((np.asarray(c.v, F32) * sv).astype(F32), sat)
            qd = e4m3((np.asarray(c.d, F32) * (F32(128.0) if mutant == "fp8_scale_128" else sd)).astype(F32), sat)
            acc0 = (x * F32(sv * sd)).astype(F32) if xacc else None
            acc = (emu_contract(qv, qd.T, "raw", acc0, cm) * so).astype(F32)
        r = acc
        dl = F32(c.delta)
        if not xacc or mutant == "x_twice":
            if mutant == "pixel_before_delta" and c.pixel:
                r = np.clip(r, F32(0), F32(1))
            if c.delta >= 0 and mutant != "delta_after_x":
                r = np.clip(r, -dl, dl)
            if x is not None:
                r = (r + x).astype(F32)
            if c.delta >= 0 and mutant == "delta_after_x":
                r = np.clip(r, -dl, dl)
        if c.pixel and mutant != "pixel_before_delta":
            r = np.clip(r, F32(0), F32(1))
        if c.stream == "bf16":
            r = trunc_bf16(r) if mutant == "trunc_out" else rne_bf16(r)
    # the output as rows of a sentinel buffer of round_up(B, 32) rows: the kernels compute whole 32-row blocks (rows >= B
    # from the clamped row B - 1) and must store rows < B only
    buf = np.full((round_up(b, 32), p), SENTINEL, F32)
    buf[:b] = r
    if mutant == "row_ge_B_stored":
        buf[b:] = r[b - 1]
    return dict(out=buf[:b].copy(), clean=bool((buf[b:] == SENTINEL).all()))


# ------------------------------------------------------------------------------------------------------ operand generators
def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def _exact_bits(rng, nbits, shape):
    """Odd integers with exactly `nbits` significant bits (top and lowest bit set), random sign, as float64."""
    if nbits == 1:
        mag = np.ones(shape, np.int64)
    else:
        mag = (1 << (nbits - 1)) | 1 | (rng.integers(0, 1 << max(nbits - 2, 0), size=shape).astype(np.int64) << 1)
    return (mag * rng.choice([-1, 1], size=shape)).astype(np.float64)


def grid_x(rng, b, p):
    """x in {0..128}/128 with the ends over-represented: sums below 0 and above 1 occur under every perturbation."""
    k = rng.integers(0, 129, size=(b, p))
    ends = rng.random((b, p))
    k = np.where(ends < 0.1, 0, np.where(ends > 0.9, 128, k))
    return (k / 128.0).astype(F32)


NARROW_QD, NARROW_QV = 2.0 ** -7, 2.0 ** -7
NARROW_DELTA = 192 * 2.0 ** -14                  # 0.01171875: on the grid, about the product's delta_clamp = 0.01


def narrow_dv(rng, p, k, b):
    """D = i 2^-7, |i| <= 127 (7 bits); V = j 2^-7, |j| <= 7: products are multiples of 2^-14, |V D^T| ~ 0.02 sqrt(K)."""
    d = _ints(rng, -127, 127, (p, k)) * NARROW_QD
    v = _ints(rng, -7, 7, (b, k)) * NARROW_QV
    return d.astype(F32), v.astype(F32)


# mid grid: per atom (bits of D, bits of V), a + b <= 20; at most MID_NNZ non-zero codes per row: the sum stays < 1
MID_CLASSES = ((9, 9), (10, 10), (9, 11), (11, 9), (16, 4), (4, 16), (12, 8), (8, 12))
MID_NNZ = 6
MID_Q = 2.0 ** -23


def mid_dv(rng, p, k, b):
    """Atom k has class (a, b) = MID_CLASSES[(k + shift) % 8]: D[:, k] = odd a-bit integers 2^-a (|D| < 1), V[:, k] = odd
    b-bit integers 2^(a - 23): every product is a multiple of 2^-23 below 2^-3, and a row of V has at most MID_NNZ
    non-zeros, so |V D^T| < 0.75 and x + V D^T < 2 = 2^24 q."""
    shift = int(rng.integers(0, 8))
    d = np.zeros((p, k))
    v = np.zeros((b, k))
    for j in range(k):
        a, bb = MID_CLASSES[(j + shift) % len(MID_CLASSES)]
        d[:, j] = _exact_bits(rng, a, p) * 2.0 ** -a
        v[:, j] = _exact_bits(rng, bb, b) * 2.0 ** (a - 23)
    keep = np.zeros((b, k), bool)
    for r in range(b):                             # row 0 is full; the last atom (last k-group, next to the padding) is in use
        n = int(rng.integers(0, MID_NNZ)) if r else MID_NNZ - 1
        keep[r, rng.permutation(k)[:n]] = True
        keep[r, k - 1] |= (r == 0) or rng.random() < 0.25
    return d.astype(F32), np.where(keep, v, 0.0).astype(F32)


WIDE_E = {"v": 2, "d": 6}                        # the partner is +-2^-e: one power per leg, so that one quantum serves the row


def wide_dv(rng, p, k, b, wide):
    """wide == "v": V = odd 24-bit integers 2^-29, every pixel's D row one-hot (+-2^-2 at one atom): q = 2^-31;
    wide == "d": D = odd 24-bit integers 2^-24, every code row one-hot (+-2^-6): q = 2^-30.  One term per output."""
    if wide == "v":
        v = _exact_bits(rng, 24, (b, k)) * 2.0 ** -29
        d = np.zeros((p, k))
        d[np.arange(p), rng.integers(0, k, size=p)] = rng.choice([-1, 1], size=p) * 2.0 ** -WIDE_E["v"]
    else:
        d = _exact_bits(rng, 24, (p, k)) * 2.0 ** -24
        v = np.zeros((b, k))
        v[np.arange(b), rng.integers(0, k, size=b)] = rng.choice([-1, 1], size=b) * 2.0 ** -WIDE_E["d"]
    return d.astype(F32), v.astype(F32)


FP8_ABSMAX = 0.75 * 2.0 ** -5                    # sc.v = 2^14, sc.v sc.d = 2^22, sc.o = 2^-22
FP8_GAUSS_ABSMAX = 8 / 255                       # the product's eps: the scales round in fp32


FP8_KINDS = ("e4m3-exact", "quantised", "saturating")
FP8_WIDTH = 12                                   # see fp8_dv


def fp8_dv(rng, p, k, b, kind):
    """The fp8 MFMA does not sum its 16 products the way the bf16 one does: with products up to 2^17 next to halves in
    one k-group an MI355X returns sums that are off by up to 4 units although they are fp32 numbers, while one repeated
    product and dense products below 2^14 come out exact (profiles/contract_exact.md): small products lose low bits
    when they are aligned to a large one.  MODEL, assumed and asserted wherever it is used: inside one k-group every
    product keeps at least FP8_WIDTH = 12 bits below the leading bit of the LARGEST product of the group.  A k-group
    whose products are multiples of q and below 2^12 q is then summed exactly.

    e4m3-exact  v sc.v = integers |m| <= 15 and 256 d = m 2^e (|m| <= 15, e <= 3) are e4m3 values; products are integers
                up to 15 * 120 < 2^11.
    quantised   dense, every operand a TIE: v sc.v = odd integers 17..31 (e4m3 spacing 2 there) and 256 d = integers + 1/2
                in 8.5..15.5 (spacing 1); the reference quantises them; products are at most 32 * 16 = 2^9, quantum 1.
    saturating  v sc.v = odd integers up to 575 (beyond 448 they saturate), 256 d = integers + 1/2 up to 240.5, and ONE
                non-zero code per k-group of 16 atoms: one product per MFMA, which needs no model of its sum."""
    sv = float(fp8_scales(FP8_ABSMAX)[0])
    sign = lambda shape: rng.choice([-1, 1], size=shape)
    if kind == "e4m3-exact":
        v = _ints(rng, -15, 15, (b, k))
        d = _ints(rng, -15, 15, (p, k)) * 2.0 ** _ints(rng, 0, 3, (p, k))
    elif kind == "quantised":
        v = (2 * _ints(rng, 8, 15, (b, k)) + 1) * sign((b, k))
        d = (_ints(rng, 8, 15, (p, k)) + 0.5) * sign((p, k))
    else:
        v = np.zeros((b, k))
        for g0 in range(0, k, KGROUP):
            col = rng.integers(g0, min(g0 + KGROUP, k), size=b)
            v[np.arange(b), col] = (2 * _ints(rng, 0, 287, b) + 1) * sign(b)
        d = (_ints(rng, 0, 240, (p, k)) + 0.5) * sign((p, k))
    return (d / 256.0).astype(F32), (v / sv).astype(F32)


def fp8_group_max(c):
    """(sum over k-groups of, max over k-groups of) the largest |product| of the group, per output, in image units; and the
    largest number of non-zero products any output has in one group."""
    v, d = synth_operands64(c)
    k = v.shape[1]
    tot = np.zeros((v.shape[0], d.shape[0]))
    top = np.zeros_like(tot)
    nnz = 0
    for g0 in range(0, k, KGROUP):
        pr = np.abs(v[:, None, g0:g0 + KGROUP] * d[None, :, g0:g0 + KGROUP])
        m = pr.max(axis=2)
        tot += m
        top = np.maximum(top, m)
        nnz = max(nnz, int((pr != 0).sum(axis=2).max()))
    return tot, top, nnz


def gauss_dv(rng, p, k, b):
    d = rng.uniform(-1, 1, (p, k)).astype(F32)
    v = (0.02 * rng.standard_normal((b, k))).astype(F32)
    return d, v


# ----------------------------------------------------------------------------------------------------------------- the rows
class SynthRow(NamedTuple):
    stream: str
    k: int
    p: int
    b: int
    off: int = 0       # elements past a 16-byte boundary (x and out in turn)


# Every K of {1, 16, 17, 33, 50, 64, 65, 100, 128} (odd / even / K % 4 == 0 fill_dict_slice branches; HOIST = 4 | 8 and 4 | 8
# waves either side of Kp = 64), every P of {432: three FAST tiles + tail, 384: all FAST, 100: one element-wise tile,
# 50: P % 4 != 0, nothing FAST} and every B of {1, 31, 33, 70, 257: a wave takes a second and third batch block}, per
# stream type.  Every row runs all five variants, i.e. both the XACC and the non-XACC kernels.
SYNTH_KPB = ((1, 432, 70), (16, 384, 31), (17, 100, 33), (33, 50, 257), (50, 432, 1), (64, 384, 257), (65, 100, 70),
             (100, 50, 31), (100, 384, 33), (128, 432, 257))
SYNTH_ROWS = [SynthRow(s, k, p, b) for s in ("f32", "bf16") for k, p, b in SYNTH_KPB]
# variant: (with x, delta_clamp, pixel_clamp); XACC <=> with x and delta_clamp < 0
SYNTH_VARIANTS = {"x+vD": (True, -1.0, False), "delta": (True, NARROW_DELTA, False), "pixel": (True, -1.0, True),
                  "both": (True, NARROW_DELTA, True), "x=None": (False, -1.0, False)}
SYNTH_GRIDS = {"f32": ("narrow", "mid", "wide_v", "wide_d"), "bf16": ("narrow", "mid")}
# fp8 rows (both stream types): packed needs P % 128 == 0 and K % 4 == 0
FP8_KPB = ((64, 384, 33), (100, 384, 70), (17, 432, 31), (50, 100, 257))
FP8_ROWS = [SynthRow(s, k, p, b) for s in ("f32", "bf16") for k, p, b in FP8_KPB]
SYNTH_GAUSS_KPB = ((50, 432, 70), (100, 384, 33), (128, 100, 257))
SYNTH_GAUSS_ROWS = [SynthRow(s, k, p, b) for s in ("f32", "bf16") for k, p, b in SYNTH_GAUSS_KPB]
STORE_ROWS = [SynthRow(s, k, p, b) for s in ("f32", "bf16") for k, p, b in ((17, 8, 33), (64, 384, 70), (100, 432, 257))]


def synth_row_id(r):
    return f"synth-{r.stream}-K{r.k}-P{r.p}-B{r.b}" + (f"-off{r.off}" if r.off else "")


def synth_cases(r, grid):
    """The calls of one row on one grid: five variants (wide grids: x = None and x = 0, the only x that leaves a 24-bit
    output exact), each at the row's placements (an offset puts x and out in turn off the 16-byte boundary)."""
    rid = f"{synth_row_id(r)}-{grid}"
    rng = np.random.default_rng(seed_of(rid))
    if grid == "narrow":
        d, v = narrow_dv(rng, r.p, r.k, r.b)
        q = NARROW_QD * NARROW_QV
    elif grid == "mid":
        d, v = mid_dv(rng, r.p, r.k, r.b)
        q = MID_Q
    elif grid in ("wide_v", "wide_d"):
        d, v = wide_dv(rng, r.p, r.k, r.b, grid[-1])
        q = 2.0 ** -31 if grid == "wide_v" else 2.0 ** -30      # 2^-29 2^-2 | 2^-24 2^-6
    else:
        raise ValueError(grid)
    wide = grid.startswith("wide")
    x = np.zeros((r.b, r.p), F32) if wide else grid_x(rng, r.b, r.p)
    variants = {"x=0": (True, -1.0, False), "x=None": (False, -1.0, False)} if wide else SYNTH_VARIANTS
    cases = []
    for vname, (with_x, delta, pixel) in variants.items():
        places = [(0, 0)] if not r.off else ([(r.off, 0), (0, r.off)] if with_x else [(0, r.off)])
        for x_off, out_off in places:
            cases.append(SynthCase(f"{rid}-{vname}-x{x_off}-o{out_off}", x if with_x else None, d, v, r.stream, delta, pixel,
                                   x_off=x_off, out_off=out_off, q=q))
    return cases


def low_quantum(a, axis):
    """The value of the lowest set bit among the non-zero elements of a float64 array along `axis` (inf if all are 0):
    every element is a multiple of it."""
    mant, ex = np.frexp(np.abs(a))
    i = np.rint(mant * 2.0 ** 53).astype(np.int64)
    low = np.where(i != 0, np.ldexp((i & -i).astype(np.float64), ex - 53), np.inf)
    return low.min(axis=axis)


def assert_premise(c, ref, s):
    """The exact legs' premise, on the reference alone, in float64: every term V[b, k] D[p, k] (operands as multiplied)
    is a multiple of q, x and an active delta are multiples of q, and sum |terms| + |x| < 2^24 q.  Every partial sum of
    the kernel, in any order, is then a multiple of q below 2^24 q: an fp32 number."""
    v, d = synth_operands64(c)
    term_q = low_quantum(v, 0) * low_quantum(d, 0)                  # per atom; inf where a column is all zero
    assert (term_q >= c.q).all(), f"{c.name}: a product is not a multiple of q"
    if c.x is not None:
        assert np.array_equal(np.rint(c.x / c.q) * c.q, c.x.astype(np.float64)), f"{c.name}: x is not on the grid"
    if c.delta >= 0:
        dl = float(F32(c.delta))
        assert dl == c.delta and np.rint(dl / c.q) * c.q == dl, f"{c.name}: delta is not on the grid"
    assert float(s.max()) < 2.0 ** 24 * c.q, f"{c.name}: sum |terms| + |x| = {float(s.max())} >= 2^24 q"
    assert np.array_equal(np.rint(ref / c.q) * c.q, ref), c.name


def check_synth_case(c, run):
    """run(case) -> dict(out float32 (B, P), clean: nothing outside `out` was written).  Bits of an exact case."""
    ref, s = ref_synth(c)
    assert_premise(c, ref, s)
    want = round_stream(ref, c.stream, c.name)
    got = run(c)
    assert got["clean"], f"{c.name}: written outside the tensor"
    assert_bits_equal(got["out"], want, c.name, ignore_zero_sign=True)
    return want


def check_synth_exact(r, grid, run):
    for c in synth_cases(r, grid):
        check_synth_case(c, run)


def fp8_cases(r, kind):
    rid = f"{synth_row_id(r)}-fp8-{kind}"
    rng = np.random.default_rng(seed_of(rid))
    d, v = fp8_dv(rng, r.p, r.k, r.b, kind)
    x = grid_x(rng, r.b, r.p)
    sv, sd, so = (float(t) for t in fp8_scales(FP8_ABSMAX))
    delta = 2.0 ** 14 * so                         # 2^-8: on the grid of the scaled-back sums (quantum sc.o = 2^-22)
    for vname, (with_x, dl, pixel) in SYNTH_VARIANTS.items():
        yield SynthCase(f"{rid}-{vname}", x if with_x else None, d, v, r.stream, delta if dl >= 0 else -1.0, pixel,
                        fp8=FP8_ABSMAX, q=so / 2 if kind == "saturating" else so)


def check_synth_fp8(r, kind, run):
    """adil_synth_fp8 on the fp8 grid, bits; and adil_synth_fp8_packed on dict_to_fp8(d) where the shape allows it: the
    same bits again.  Beside the premise of every exact row, the fp8 model's: one product per k-group, or every product
    of a k-group below 2^FP8_WIDTH q."""
    sv, sd, _ = fp8_scales(FP8_ABSMAX)
    for c in fp8_cases(r, kind):
        _, top, nnz = fp8_group_max(c)
        assert nnz == 1 or float(top.max()) < 2.0 ** FP8_WIDTH * c.q, f"{c.name}: outside the fp8 summation model"
        if kind == "quantised":                    # every operand is a tie of the e4m3 conversion
            assert (e4m3(c.v * sv) != c.v * sv).all() and (e4m3(c.d * sd) != c.d * sd).all()
        if kind == "saturating":
            assert (e4m3(c.v * sv) != c.v * sv).any() and (e4m3(c.d * sd) != c.d * sd).any() and (np.abs(c.v * sv) > 448).any()
        want = check_synth_case(c, run)
        if r.p % 128 == 0 and r.k % 4 == 0:
            got = run(c._replace(packed=True))
            assert got["clean"], f"{c.name} packed: written outside the tensor"
            assert_bits_equal(got["out"], want, f"{c.name} packed", ignore_zero_sign=True)


def gauss_bound(c, ref, s):
    """|out - r| <= u_T (|r| + A) + A (+ 2^-24 |r| for the fp32 sum clamp(acc) + x of an active delta clamp), elementwise.

    S = |V| |D|^T + |x| in float64 on the operands as multiplied, n = K terms (+ 1 for x in the accumulator).
    bf16 streams: the products of bf16 operands are exact in fp32 and the accumulator is fp32: n additions in any order
    lose at most n 2^-24 S (first order); the factor c = 2 covers the MFMA's internal summation of its 16 terms, whose
    order and intermediate rounding the ISA does not state (as in classifier_reference.py): A = 2 n 2^-24 S.
    fp32 streams: the six piece products are exact and accumulate the same way (the lower pieces add roundings on
    partial sums no larger than S: the same A), and three of the nine piece products are never issued: |am bl| + |al bm| +
    |al bl| <= (2^-9 2^-17 + 2^-17 2^-9 + 2^-34) |a b| < 2^-24 |a b|; the split itself is exact for fp32 operands (three
    bf16 pieces hold 24 bits), the issue's allowance of 2^-25 per operand is kept: A = 2 n 2^-24 S + 2^-23 S.
    fp8: the reference multiplies the operands the kernel multiplies — e4m3(f32(v sc.v)), e4m3(f32(256 d)), the scales
    formed in fp32 as fp8_scale() forms them, both conversions correctly rounded fp32 products — so the quantisation is
    not an error term; x sc.v sc.d and acc sc.o each round once more (n + 2 in place of n).  The MFMA's own sum follows
    the model of fp8_dv: in each k-group each of the 16 products loses less than 2^-12 of the group's largest product
    M_g, so A grows by 16 2^-12 sum_g M_g (in image units).  That term is about 2^-10 S: it dominates A on fp32 streams.
    Both clamps are 1-Lipschitz, so a bound on the accumulator carries through them.  The store rounds to the stream
    type: u_T = 2^-8 (bf16) | 2^-24 (fp32) relative to the value it rounds, which is within A of r."""
    n = c.d.shape[1] + (1 if c.x is not None else 0) + (2 if c.fp8 is not None else 0)
    a = 2.0 * n * U24 * s
    if c.fp8 is not None:
        a = a + 16 * 2.0 ** -FP8_WIDTH * fp8_group_max(c)[0]
    elif c.stream == "f32":
        a = a + 2.0 ** -23 * s
    ut = 2.0 ** -8 if c.stream == "bf16" else U24
    bound = ut * (np.abs(ref) + a) + a
    if c.delta >= 0 and c.x is not None:
        bound = bound + U24 * np.abs(ref)
    return bound


GAUSS_DELTA = 0.01


def gauss_cases(r, fp8=False):
    rid = f"{synth_row_id(r)}-gauss" + ("-fp8" if fp8 else "")
    rng = np.random.default_rng(seed_of(rid))
    d, v = gauss_dv(rng, r.p, r.k, r.b)
    x = rng.uniform(0, 1, (r.b, r.p)).astype(F32)
    if r.stream == "bf16":
        x = rne_bf16(x)
    if fp8:
        v = np.clip(v, -FP8_GAUSS_ABSMAX, FP8_GAUSS_ABSMAX).astype(F32)
    for vname, (with_x, dl, pixel) in SYNTH_VARIANTS.items():
        yield SynthCase(f"{rid}-{vname}", x if with_x else None, d, v, r.stream, GAUSS_DELTA if dl >= 0 else -1.0, pixel,
                        fp8=FP8_GAUSS_ABSMAX if fp8 else None)


def check_synth_gauss(r, run, fp8=False):
    """Gaussian operands against float64 within gauss_bound; returns the worst err / bound over the five variants.
    fp8: fp8_absmax = 8/255, codes clipped to it; also through adil_synth_fp8_packed where the shape allows it."""
    worst = 0.0
    for c in gauss_cases(r, fp8):
        ref, s = ref_synth(c)
        got = run(c)
        assert got["clean"], f"{c.name}: written outside the tensor"
        bound = gauss_bound(c, ref, s)
        worst = max(worst, assert_within(got["out"], ref, bound, c.name))
        if fp8 and r.p % 128 == 0 and r.k % 4 == 0:
            got = run(c._replace(packed=True))
            assert got["clean"], f"{c.name} packed: written outside the tensor"
            worst = max(worst, assert_within(got["out"], ref, bound, f"{c.name} packed"))
    return worst


# ------------------------------------------------------------------------------------------------------------- synth_store
def store_operands(r):
    """An 8-bit store of max(9, 256 / P) rows that holds every byte, and an index that gathers EVERY row (so every byte
    reaches the kernel), out of order, and then repeats some."""
    rng = np.random.default_rng(seed_of(synth_row_id(r) + "-store"))
    nrows = max(9, -(-256 // r.p))
    assert r.b > nrows
    store = rng.integers(0, 256, size=(nrows, r.p), dtype=np.uint8)
    flat = store.reshape(-1)
    flat[rng.permutation(flat.size)[:256]] = np.arange(256, dtype=np.uint8)
    index = np.concatenate([rng.permutation(nrows), rng.integers(0, nrows, size=r.b - nrows)]).astype(np.int64)
    assert np.unique(store[index]).size == 256 and np.unique(index).size < index.size and (np.diff(index) < 0).any()
    d, v = narrow_dv(rng, r.p, r.k, r.b)
    return store, index, d, v


def check_synth_store(r, run_store):
    """run_store(store, index, case) -> dict(out, gathered, clean): adil_synth_store, and adil_synth on the gathered rows
    (`gathered` is None on bf16 streams).  x = u / 255 is a 24-bit fp32 number, so x + V D^T is not exact: the outputs of
    both stream types are held to float64 of u8_unit(u) + V D^T within gauss_bound (V, D on the narrow grid), and the fp32
    output must be the bits of synth(gather_images(store, index), ...).  Returns the worst err / bound."""
    store, index, d, v = store_operands(r)
    x = (store[index].astype(F32) / F32(255.0)).astype(F32)        # u8_unit: correctly rounded u / 255
    worst = 0.0
    for vname, (with_x, dl, pixel) in SYNTH_VARIANTS.items():
        if not with_x:
            continue
        c = SynthCase(f"{synth_row_id(r)}-store-{vname}", x, d, v, r.stream, dl, pixel)
        ref, s = ref_synth(c)
        got = run_store(store, index, c)
        assert got["clean"], f"{c.name}: written outside the tensor"
        worst = max(worst, assert_within(got["out"], ref, gauss_bound(c, ref, s), c.name))
        if r.stream == "f32":
            assert_bits_equal(got["out"], got["gathered"], f"{c.name}: store against synth(gather_images)")
    return worst


# =================================================================================================================== z-step
class ZRow(NamedTuple):
    b: int
    p: int
    k: int
    off: int = 0       # z, m, s in turn `off` elements past a 16-byte boundary
    dyn: bool = False  # step_size / bc2_sqrt from device memory, bogus values from the host


Z_EPS = 0.02
Z_LR = 1e-2
Z_STEPS = 3


def zrow_id(r):
    return f"zstep-B{r.b}-P{r.p}-K{r.k}" + (f"-off{r.off}" if r.off else "") + ("-dyn" if r.dyn else "")


def emu_zstep(z, m, s, dpt, gv, h, lo, hi, mutant=None, codes=False):
    """zstep_mfma_kernel / zstep_codes_kernel: gz = gv D_dagger (dpt is D_dagger^T, (P, K)) on the six-product path,
    adamw_elem, the clamp, max |z_new - z|; codes: v' = z_new D_dagger^T on the same path in k-groups of 32 pixels.
    mutants (beside emu_contract's): delta_before_clamp | codes_from_old_z."""
    cm = mutant if mutant in DROP_MUTANTS + ("swap_ml", "skip_last_group", "pad_not_zeroed") else None
    gz = emu_contract(gv, np.asarray(dpt, F32).T, "f32", None, cm)
    q, m1, s1, delta, small = U.adamw_elem_f32(z, gz, m, s, h, lo, hi, mutant if mutant == "delta_before_clamp" else None)
    out = dict(z=q, m=m1, s=s1, delta=delta, smallest=small, clean=True)
    if codes:
        out["codes"] = emu_contract(z if mutant == "codes_from_old_z" else q, dpt, "f32", None, cm, kgroup=32)
    return out


def zstep_operands(r, grid):
    """dpt (P, K) = D_dagger^T with a third of its pixel rows zero (gz = 0 there, exactly), the per-step code gradients
    gv_it = gv 2^-it (still on the grid), gaussian z0 ~ 0.01 N(0,1), and the quantum of gz."""
    rng = np.random.default_rng(seed_of(f"{zrow_id(r)}-{grid}"))
    if grid == "narrow":                            # gv = i 2^-3, D_dagger = j 2^-7, |i|, |j| <= 15: q = 2^-10 (2^-12 at step 3)
        gv = (_ints(rng, -15, 15, (r.b, r.k)) * 2.0 ** -3).astype(F32)
        dpt = (_ints(rng, -15, 15, (r.p, r.k)) * 2.0 ** -7).astype(F32)
        q = 2.0 ** -10
    else:
        dpt, gv = mid_dv(rng, r.p, r.k, r.b)
        q = MID_Q
    dpt[rng.permutation(r.p)[: r.p // 3]] = 0.0
    z0 = (0.01 * rng.standard_normal((r.b, r.p))).astype(F32)
    return dpt, [(gv * F32(0.5 ** it)).astype(F32) for it in range(Z_STEPS)], z0, q


def ref_gz(gv, dpt, q, what):
    """gz in float64 with the exact legs' premise: sum |terms| < 2^24 q', q' the quantum of this step's terms."""
    g64, d64 = gv.astype(np.float64), dpt.astype(np.float64)
    term_q = low_quantum(g64, 0) * low_quantum(d64, 0)
    assert (term_q >= q).all(), f"{what}: a product is not a multiple of q"
    assert float((np.abs(g64) @ np.abs(d64).T).max()) < 2.0 ** 24 * q, f"{what}: sum |terms| >= 2^24 q"
    gz = g64 @ d64.T
    assert np.array_equal(gz.astype(F32).astype(np.float64), gz)
    return gz.astype(F32)


def check_zstep(r, grid, run):
    """run(z, m, s, dpt, gv, h, lo, hi, dyn, off) -> dict(z, m, s, delta, clean); h is what the host passes, dyn the two
    step-dependent scalars for the device buffer (or None), off = {"z": .., "m": .., "s": ..} element offsets.
    Three steps of AdamWSchedule(1e-2): z, m, s and max |dz| are the bits of adamw_elem_f32 on the exact gz + clamp after
    every step."""
    dpt, gvs, z0, q = zstep_operands(r, grid)
    for moved in (("z", "m", "s") if r.off else (None,)):
        off = {n: (r.off if n == moved else 0) for n in "zms"}
        z, m, s = z0.copy(), np.zeros_like(z0), np.zeros_like(z0)
        for it, gv in enumerate(gvs):
            what = f"{zrow_id(r)}-{grid} step {it + 1}, {moved or 'nothing'} unaligned"
            gz = ref_gz(gv, dpt, q * 0.5 ** it, what)
            h = U.adamw_hyper(Z_LR, it + 1)
            wz, wm, ws, wdelta, small = U.adamw_elem_f32(z, gz, m, s, h, -Z_EPS, Z_EPS)
            assert small >= U.TINY, ("subnormal intermediate in the reference", small)
            host_h = h[:4] + U.BOGUS if r.dyn else h
            got = run(z.copy(), m.copy(), s.copy(), dpt, gv, host_h, -Z_EPS, Z_EPS, (h[4], h[5]) if r.dyn else None, off)
            assert got["clean"], f"{what}: written outside a tensor"
            for key, want in (("z", wz), ("m", wm), ("s", ws)):
                assert_bits_equal(got[key], want, f"{what}: {key}")
            assert_bits_equal(F32(got["delta"]), wdelta, f"{what}: max_abs_delta")
            z, m, s = wz, wm, ws


def zstep_vacuity(r, grid):
    """Shares, on the reference alone: gz == 0, the clamp binds (at either end), after the first step."""
    dpt, gvs, z0, q = zstep_operands(r, grid)
    gz = ref_gz(gvs[0], dpt, q, "vacuity")
    wz = U.adamw_elem_f32(z0, gz, np.zeros_like(z0), np.zeros_like(z0), U.adamw_hyper(Z_LR, 1), -Z_EPS, Z_EPS)[0]
    return dict(gz_zero=float((gz == 0).mean()), clamp_binds=float((np.abs(wz) == F32(Z_EPS)).mean()))


def _zrow_of(route):
    b, c, h, w, k = route.shape
    return ZRow(b, c * h * w, k, route.offset)


# the zstep rows of test_gpu_routes.ROUTES, and three more
Z_ROUTE_ROWS = [_zrow_of(r) for r in ROUTES if r.entry == "zstep"]
Z_ROWS = Z_ROUTE_ROWS + [ZRow(33, 768, 50), ZRow(257, 432, 10), ZRow(33, 768, 50, dyn=True)]

# -------------------------------------------------------------------------------------------------------------- zstep_codes
ZC_ROWS = [_zrow_of(r) for r in ROUTES if r.entry == "zstep_codes"]
ZC_CLAMP = 2.0 ** -6
ZC_LR = 1.0                                        # a step of about +-1 against a clamp of 2^-6: every moving z saturates


def check_zstep_codes(r, run_codes, run_zstep):
    """run_codes(z, m, s, dpt, gv, h, lo, hi, dyn, off) -> dict(z, m, s, delta, codes (B, K), clean) through
    adil_zstep_codes + pack_codes; run_zstep: adil_zstep on the same operands.

    exact       three steps on the narrow grid: z, m, s, max |dz| are the bits of the reference AND of adil_zstep;
    saturating  lr = 1 against a clamp of +-2^-6, z0 = 0 where gz = 0: every z_new is -sign(gz) 2^-6 or 0 (asserted on the
                reference), so the codes z_new D_dagger^T are sums of multiples of 2^-13: bits;
    gaussian    D_dagger ~ 0.1 N(0,1), gv ~ N(0,1): the codes against the float64 product of the kernel's OWN z output
                (held to the bit by the legs above) within codes_bound.  Returns the worst err / bound."""
    rid = zrow_id(r).replace("zstep", "zstep_codes")
    no_off = dict(z=0, m=0, s=0)
    # exact
    dpt, gvs, z0, q = zstep_operands(r, "narrow")
    z, m, s = z0.copy(), np.zeros_like(z0), np.zeros_like(z0)
    for it, gv in enumerate(gvs):
        what = f"{rid} step {it + 1}"
        gz = ref_gz(gv, dpt, q * 0.5 ** it, what)
        h = U.adamw_hyper(Z_LR, it + 1)
        wz, wm, ws, wdelta, small = U.adamw_elem_f32(z, gz, m, s, h, -Z_EPS, Z_EPS)
        assert small >= U.TINY
        got = run_codes(z.copy(), m.copy(), s.copy(), dpt, gv, h, -Z_EPS, Z_EPS, None, no_off)
        other = run_zstep(z.copy(), m.copy(), s.copy(), dpt, gv, h, -Z_EPS, Z_EPS, None, no_off)
        assert got["clean"], what
        for key, want in (("z", wz), ("m", wm), ("s", ws)):
            assert_bits_equal(got[key], want, f"{what}: {key}")
            assert_bits_equal(got[key], other[key], f"{what}: {key} against adil_zstep")
        assert_bits_equal(F32(got["delta"]), wdelta, f"{what}: max_abs_delta")
        assert_bits_equal(F32(got["delta"]), F32(other["delta"]), f"{what}: max_abs_delta against adil_zstep")
        z, m, s = wz, wm, ws
    # saturating step
    z = np.where(ref_gz(gvs[0], dpt, q, rid) != 0, z0, F32(0)).astype(F32)
    m, s = np.zeros_like(z), np.zeros_like(z)
    for it in range(2):
        what = f"{rid} saturating step {it + 1}"
        gz = ref_gz(gvs[0], dpt, q, what)
        h = U.adamw_hyper(ZC_LR, it + 1)
        wz, wm, ws, wdelta, small = U.adamw_elem_f32(z, gz, m, s, h, -ZC_CLAMP, ZC_CLAMP)
        assert small >= U.TINY
        assert np.array_equal(wz, (-np.sign(gz) * ZC_CLAMP).astype(F32)), f"{what}: the step does not saturate"
        codes = wz.astype(np.float64) @ dpt.astype(np.float64)      # multiples of 2^-13, |sum| <= P 15 2^-13
        assert float((np.abs(wz.astype(np.float64)) @ np.abs(dpt.astype(np.float64))).max()) < 2.0 ** 24 * 2.0 ** -13
        got = run_codes(z.copy(), m.copy(), s.copy(), dpt, gvs[0], h, -ZC_CLAMP, ZC_CLAMP, None, no_off)
        assert got["clean"], what
        for key, want in (("z", wz), ("m", wm), ("s", ws)):
            assert_bits_equal(got[key], want, f"{what}: {key}")
        assert_bits_equal(F32(got["delta"]), wdelta, f"{what}: max_abs_delta")
        assert_bits_equal(got["codes"], codes.astype(F32), f"{what}: codes", ignore_zero_sign=True)
        z, m, s = wz, wm, ws
    # gaussian
    rng = np.random.default_rng(seed_of(rid + "-gauss"))
    dpt = (0.1 * rng.standard_normal((r.p, r.k))).astype(F32)
    gv = rng.standard_normal((r.b, r.k)).astype(F32)
    z = (0.01 * rng.standard_normal((r.b, r.p))).astype(F32)
    got = run_codes(z, np.zeros_like(z), np.zeros_like(z), dpt, gv, U.adamw_hyper(Z_LR, 1), -Z_EPS, Z_EPS, None, no_off)
    assert got["clean"], rid
    zn = _np(got["z"]).astype(np.float64)
    ref = zn @ dpt.astype(np.float64)
    return assert_within(got["codes"], ref, codes_bound(np.abs(zn) @ np.abs(dpt.astype(np.float64)), r.p), f"{rid}: gaussian codes")


def codes_bound(s, p, nslabs=256):
    """|codes - r| <= A = 2 n 2^-24 S + 2^-23 S, n = P terms plus the additions of the slab sum (at most one per slab: a
    slab per workgroup, at most one workgroup per compute unit, 256 of them), S = |z_new| |D_dagger^T|: the fp32-stream
    bound of gauss_bound without an output rounding (the codes stay fp32)."""
    return 2.0 * (p + nslabs) * U24 * s + 2.0 ** -23 * s
