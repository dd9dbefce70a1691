"""What the strided dense kernels (adil_dense1x1_fwd_ld / _bwd_ld, adil_dense3x3_fwd_ld / _bwd_ld) and `ops.dense_block`
add to tests/dense1x1_reference.py and tests/dense3x3_reference.py, which are imported and left as they are: the tables of
the strided tests, the restatement of `accumulate = 1`, its operand `old`, and an fp64 restatement of a whole dense block.
Plain torch; CPU or GPU.

    accumulate   gx[m][k] = bf16_rne(f32(old[m][k]) + v),  v = t * pscale[k] (one fp32 product) where pre[m][k] > 0, else +0:
                 ONE fp32 add, ONE rounding.  As a D1Out: pre = where(keep, t * pscale, 0) + old, S = S_bwd + |old|,
                 n = N + 2 (the N products, the product by pscale, the add), keep = None (the mask is inside pre: a masked
                 element is old + 0, and -0.0 + 0 = +0), so compare_exact / assert_premise / gaussian_ratio of
                 dense1x1_reference apply unchanged.
    exact legs   `old` is integer-valued bf16: a multiple of the quantum 1/4, so old + v is exact in fp32 under the premise
                 sum |terms| < 2^23 quanta (S includes |old|) and the one correct output is the RNE rounding of the exact
                 sum.  |old| <= OLD_AMP[leg]; on the rounding set the range is chosen so that rounding v to bf16 BEFORE the
                 add (the double-rounding mutant) changes at least 1 % of the reference's outputs
                 (tests/test_dense_block_cpu.py asserts it on the reference alone).
    gaussian leg old ~ N(0, 1) rounded to bf16; the bound is dense1x1_reference's with the S and n above."""
import functools

import torch

import dense1x1_reference as d1
import dense3x3_reference as d3
from classifier_reference import BF16, F32, F64, Arith, bf16_rne, rng  # noqa: F401

# (M, K, N, act, ld): ld is the row pitch of the K-wide operands (x, xin, gx); the N-wide ones (y, g) get N + 8.
# (129, 96, 128): K is no multiple of 64 and the 16-byte chunk past K lies INSIDE the row, where the neighbouring slice
# lives; (300, 512, 256): ld equals the width
D1_LD_ROWS = [(1, 8, 8, 1, 16), (127, 24, 40, 0, 72), (129, 96, 128, 1, 160), (300, 64, 128, 1, 256), (200, 992, 128, 1, 1024),
              (300, 512, 256, 0, 512)]
# (B, H, W, C, N): the 32-wide side lives at channel offset D3_OFF of a D3_LD-wide buffer, the other side has pitch
# width + 8.  196 pixels: less than one tile; 800: several tiles, halo rows of a neighbouring tile
D3_LD_ROWS = [(2, 7, 7, 128, 32), (1, 14, 14, 128, 32), (2, 20, 20, 128, 32), (3, 6, 10, 64, 32), (1, 3, 63, 32, 64)]
D3_OFF, D3_LD = 96, 256
MASK_ROW = d3.MASK_ROW
# |old| of the exact legs, integers
OLD_AMP = {"clamp": 4, "rounding": 2048}

NEW_SYMBOLS = {"adil_dense1x1_fwd_ld": 14, "adil_dense1x1_bwd_ld": 18, "adil_dense3x3_fwd_ld": 11, "adil_dense3x3_bwd_ld": 11}


def row_name(M, K, N, act, ld):
    return d1.row_name(M, K, N, act) + "-ld%d" % ld


def old_operand(name, leg, M, K):
    """The gradient already in gx [M][K] bf16: integers of both signs (zeros and, on the first row, -0.0 included) on the
    exact legs, N(0, 1) on the gaussian leg."""
    gen = rng(name + "/old", leg)
    if leg == "gaussian":
        return torch.randn(M, K, generator=gen).to(BF16)
    amp = OLD_AMP[leg]
    old = torch.randint(-amp, amp + 1, (M, K), generator=gen).float()
    old = bf16_rne(old)                                                  # integers beyond 256 keep 8 bits
    old[0, ::2] = -0.0                                                   # an old -0.0: +0 under a masked element
    return old.to(BF16)


def accumulate(ar, bwd, old, mut=()):
    """The D1Out of gx after adil_dense1x1_bwd_ld(accumulate = 1) from the D1Out `bwd` of d1_bwd in the same arithmetic.
    mut: 'double_round' (v rounded to bf16 before the add), 'ignored' (accumulate = 0), 'no_mask' (the mask dropped on the
    added value), 'row_old' (the old value of the next row)."""
    dt = ar.dtype
    v = ar.rnd(bwd.pre) if "double_round" in mut else bwd.pre
    if bwd.keep is not None and "no_mask" not in mut:
        v = torch.where(bwd.keep, v, torch.zeros_like(v))
    o = old.to(dt)
    if "row_old" in mut:
        o = torch.roll(o, -1, 0)
    pre = v if "ignored" in mut else v + o
    S = bwd.S + old.to(dt).abs() if ar.ref else None
    return d1.D1Out(pre, S, bwd.n + 1, False, None)


@functools.lru_cache(maxsize=None)
def reference_row(row, leg):
    """(dense1x1_reference.Row, old, reference D1Out of the accumulated gx) of one row of D1_LD_ROWS and one leg, computed
    once and shared; never modified.  The exact legs' premises are asserted on the reference alone."""
    M, K, N, act, ld = row
    name = row_name(*row)
    r = d1.reference_row(name, leg, M, K, N, act)
    old = old_operand(name, leg, M, K)
    acc = accumulate(Arith(), r.bwd, old)
    if leg != "gaussian":
        worst = float(acc.S.max()) / d1.QUANTUM
        assert worst < 2.0 ** 23, f"{name}: sum |terms| = {worst:.0f} quanta >= 2^23 with the old gradient"
        assert bool((acc.pre / d1.QUANTUM == (acc.pre / d1.QUANTUM).round()).all()), name
    return r, old, acc


def exact_leg(act):
    return d1.legs_of(act)[0]


def emulate_accumulate(row, leg, mut=()):
    """(reference tuple, the fp32 emulation's accumulated gx): fp32 arithmetic, reduction in chunks of 16."""
    M, K, N, act, ld = row
    ref = reference_row(row, leg)
    r, old, _ = ref
    em, o = Arith(F32, 16), r.ops
    bwd = d1.d1_bwd(em, o.g, r.y, o.scale, o.wt, o.x, o.pscale, o.pshift, act)
    return ref, d1.finish(em, accumulate(em, bwd, old, mut))


# ------------------------------------------------------------------------------------------------- a whole dense block
def block_fp64(block, x, g):
    """fp64 restatement of a dense block of zoo._OwnDenseLayer children (plain loop or zoo._OwnDenseBlock): the weights
    and the layers' own fp32 tables upcast, activations unrounded, torch.cat and autograd as they are.  x [B][C0][H][W],
    g the gradient of the output.  Returns (output, input gradient) in fp64."""
    F = torch.nn.functional
    up = lambda t: t.detach().to("cpu").double()
    col = lambda t: up(t).reshape(1, -1, 1, 1)
    xin = up(x).contiguous().requires_grad_(True)
    feats = [xin]
    for layer in block.values():
        t = torch.relu(torch.cat(feats, 1) * col(layer.pscale) + col(layer.pshift))
        t = F.conv2d(t, up(layer.conv1.weight))
        t = torch.relu(t * col(layer.scale) + col(layer.shift))
        feats.append(F.conv2d(t, up(layer.conv2.weight), None, 1, 1))
    out = torch.cat(feats, 1)
    (gx,) = torch.autograd.grad(out, xin, up(g))
    return out.detach(), gx
