"""Row tables, operand generators and emulations of the VGG kernels (csrc/adil_conv3x3.hip, csrc/adil_bias_relu_pool2.hip): the wide-image 3x3
convolution adil_conv3x3_wide and the bias + ReLU + 2x2 max-pool pair adil_bias_relu_pool2_fwd / _bwd.  The fp64
restatement of the convolution, the two legs and the comparators are those of tests/classifier_reference.py (`conv3x3`,
`conv3x3_bwd`, `compare_exact`, `assert_premise`, `gaussian_ratio`); nothing of them is restated here.

convolution
  exact leg     x, g integers in [-16, 16], w integers in [-8, 8]: every product and partial sum is an integer below
                9 * 512 * 16 * 8 < 2^20, exact in fp32 in any order; the outputs are compared bit for bit.
  gaussian leg  x, g ~ N(0, 1), w ~ N(0, 1 / (9 R)) with R the reduction of the direction the weight is used in, bound
                gaussian_ratio <= 1.
pool pair       the reference is torch's own fp32 chain max_pool2d(relu(x.float() + bias), 2) and its autograd on the CPU;
                the comparison is bit for bit on both legs.
  tie leg       x integers in [-4, 4], bias multiples of 0.5 in [-2, 2]: tied maxima and dead windows are common.
  gaussian leg  x ~ N(0, 1), bias ~ N(0, 0.25)."""
import functools
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from classifier_reference import (BF16, Arith, Gen, Out, assert_premise, compare_exact, conv3x3, conv3x3_bwd,  # noqa: F401
                                  finish, gaussian_ratio, pack_taps, pack_taps_flipped, rng, stats)

TW = 16                          # tile width of conv3x3_kernel on 2-D tiles (adil_conv3x3_wide)


def tile_rows(O):
    """Tile height: 8 x 16 pixels x 128 channels where the output channels are a multiple of 128, else 16 x 16 x 64."""
    return 8 if O % 128 == 0 else 16


# (B, H, W, C, N): both directions run on every row, so each row meets both tile shapes unless C and N are of one kind
ISSUE_ROWS = [
    (1, 1, 1, 64, 64),           # one pixel
    (1, 3, 64, 64, 64),          # the first width adil_conv3x3 refuses
    (2, 5, 70, 64, 128),         # width not a multiple of the tile width; two images
    (1, 17, 65, 128, 64),        # partial tiles both ways
    (1, 2, 224, 64, 64),         # the widest row of the network
    (1, 16, 112, 64, 128),       # layer 2's width and channels
    (3, 6, 10, 64, 64),          # images smaller than a tile
    (1, 63, 1, 64, 64),          # W = 1
    (1, 9, 15, 512, 64),         # the largest reductions
    (1, 9, 15, 64, 512),
]
TILE_EDGE_ROWS = [
    (1, 7, 15, 64, 128),         # 8 x 16 forward (16 x 16 gradient): TH - 1 rows, TW - 1 columns
    (1, 8, 16, 64, 128),         # TH, TW
    (1, 9, 17, 64, 128),         # TH + 1, TW + 1
    (1, 15, 15, 64, 64),         # 16 x 16: TH - 1, TW - 1
    (1, 16, 16, 64, 64),         # TH, TW
    (1, 17, 17, 64, 64),         # TH + 1, TW + 1
    (1, 8, 16, 128, 128),        # 8 x 16 in both directions: the tile
    (2, 9, 130, 128, 128),       # ... 2 x 2 x 9 = 36 pixel tiles: the XCD-swizzled map is not taken (36 % 8 != 0)
    (2, 16, 64, 128, 128),       # ... 2 x 2 x 4 = 16 pixel tiles: the XCD-swizzled map
    (1, 16, 64, 64, 256),        # 8 pixel tiles x 2 channel tiles forward: the swizzled map with more than one channel tile
]
ROWS = ISSUE_ROWS + TILE_EDGE_ROWS
NAN_ROWS = [(2, 5, 70, 64, 128), (3, 6, 10, 64, 64)]
HASH_ROWS = [(2, 5, 70, 64, 128), (1, 17, 65, 128, 64), (3, 6, 10, 64, 64)]

# (B, H, W, C, N) the entry point refuses: C or N of 32, 96 or 0; W, H or B of 0 or -1
REFUSED_DIMS = ([(2, 4, 4, c, 64) for c in (32, 96, 0)] + [(2, 4, 4, 64, n) for n in (32, 96, 0)]
                + [(2, 4, 0, 64, 64), (2, 4, -1, 64, 64), (2, 0, 4, 64, 64), (2, -1, 4, 64, 64), (0, 4, 4, 64, 64),
                   (-1, 4, 4, 64, 64)])

# (B, H, W, C) of the pool pair; each runs with and without bias
POOL_ROWS = [(1, 2, 2, 8), (2, 6, 10, 16), (1, 4, 126, 64), (1, 2, 224, 64), (3, 8, 8, 72)]
POOL_HASH_ROWS = [(2, 6, 10, 16), (3, 8, 8, 72)]
POOL_REFUSED_DIMS = [(2, 5, 4, 8), (2, 4, 5, 8), (2, 4, 4, 12), (2, 4, 4, 0), (2, 0, 4, 8), (2, 4, 0, 8), (0, 4, 4, 8),
                     (-1, 4, 4, 8), (2, -2, 4, 8)]

# (C, N, H, pooled) of VGG11's eight groups at 224 x 224, in network order
VGG11_GROUPS = [(3, 64, 224, True), (64, 128, 112, True), (128, 256, 56, False), (256, 256, 56, True),
                (256, 512, 28, False), (512, 512, 28, True), (512, 512, 14, False), (512, 512, 14, True)]


def row_name(B, H, W, C, N):
    return "conv3x3_wide/%dx%dx%d/%d->%d" % (B, H, W, C, N)


class Operands(NamedTuple):
    x: torch.Tensor              # [B][H][W][C] bf16
    g: torch.Tensor              # [B][H][W][N] bf16
    w: torch.Tensor              # [N][C][3][3] bf16: the forward's weight
    wg: torch.Tensor             # [N][C][3][3] bf16: the gradient's weight (the same tensor on the exact leg)


def operands(name, leg, B, H, W, C, N):
    gen = Gen(name, leg)
    x, g = gen.act(B, H, W, C, amp=16), gen.act(B, H, W, N, amp=16)
    w = gen.weight(N, C, 3, 3, amp=8, fan_in=9 * C)
    wg = w if leg == "exact" else gen.weight(N, C, 3, 3, amp=8, fan_in=9 * N)
    return Operands(x, g, w, wg)


class Row(NamedTuple):
    ops: Operands
    wp: torch.Tensor             # [N][9][C] bf16
    wp_bwd: torch.Tensor         # [C][9][N] bf16
    fwd: Out
    bwd: Out


@functools.lru_cache(maxsize=None)
def reference_row(row, leg):
    """Operands and fp64 reference of one row and leg, computed once and shared; never modified."""
    B, H, W, C, N = row
    op = operands(row_name(*row), leg, B, H, W, C, N)
    ar = Arith()
    return Row(op, pack_taps(op.w), pack_taps_flipped(op.wg), conv3x3(ar, op.x, op.w)["y"], conv3x3_bwd(ar, op.g, op.wg)["gx"])


def emulate(ar, src, wp, mut=()):
    """The kernel on its packed weights, as an Arith emulation of the 2-D tiling: per image and TH x 16 tile the
    (TH + 2) x 18 halo is staged with ZEROS where it leaves the image, tap (kh, kw) of tile pixel (r, c) is halo pixel
    (r + kh, c + kw), taps in the order kh * 3 + kw, and only the pixels inside the image are stored.
    src [B][H][W][R], wp [O][9][R].  Mutants:
      no_right_fill / no_bottom_fill  a halo pixel past the right / bottom edge is read at its linear address instead
                                      (the next row's first pixel / the next image's row, wrapping at the operand's end)
      origin_off_by_one               the halo starts at the tile's own first column instead of one to its left
      tap_transposed                  tap kw * 3 + kh"""
    B, H, W, R = src.shape
    O = wp.shape[0]
    TH = tile_rows(O)
    dt = ar.dtype
    flat = src.to(dt).reshape(B * H * W, R)
    out = torch.zeros(B, H, W, O, dtype=dt)
    hr, hc = torch.meshgrid(torch.arange(TH + 2), torch.arange(TW + 2), indexing="ij")
    for b in range(B):
        for h0 in range(0, H, TH):
            for w0 in range(0, W, TW):
                gh = h0 - 1 + hr
                gw = w0 - 1 + hc + (1 if "origin_off_by_one" in mut else 0)
                inside = (gh >= 0) & (gh < H) & (gw >= 0) & (gw < W)
                if "no_right_fill" in mut:
                    inside |= (gh >= 0) & (gh < H) & (gw >= W)
                if "no_bottom_fill" in mut:
                    inside |= (gh >= H) & (gw >= 0) & (gw < W)
                lin = (((b * H + gh) * W + gw) % (B * H * W)).clamp_min(0)
                halo = torch.where(inside[..., None], flat[lin], torch.zeros((), dtype=dt))
                acc = torch.zeros(TH * TW, O, dtype=dt)
                for kh in range(3):
                    for kw in range(3):
                        tap = kw * 3 + kh if "tap_transposed" in mut else kh * 3 + kw
                        rows = halo[kh:kh + TH, kw:kw + TW].reshape(TH * TW, R)
                        acc = acc + ar.mm(rows, wp[:, tap].to(dt).t())
                th, tw = min(TH, H - h0), min(TW, W - w0)
                out[b, h0:h0 + th, w0:w0 + tw] = acc.reshape(TH, TW, O)[:th, :tw]
    return finish(ar, Out(out, None, 9 * R))


def pack_bwd_unflipped(w):
    """The mutant of the gradient pack: channels swapped, taps NOT flipped."""
    return pack_taps(w.transpose(0, 1))


# ------------------------------------------------------------------------------------------------------------ pool pair
def pool_name(B, H, W, C, bias):
    return "bias_relu_pool2/%dx%dx%dx%d/%s" % (B, H, W, C, "bias" if bias else "nobias")


class PoolOperands(NamedTuple):
    x: torch.Tensor              # [B][H][W][C] bf16
    bias: Optional[torch.Tensor]  # [C] fp32 or None
    g: torch.Tensor              # [B][H/2][W/2][C] bf16


def pool_operands(name, leg, B, H, W, C, with_bias):
    gen = rng(name, leg)
    if leg == "tie":
        x = torch.randint(-4, 5, (B, H, W, C), generator=gen).to(BF16)
        bias = torch.randint(-4, 5, (C,), generator=gen).float() * 0.5
    else:
        x = torch.randn((B, H, W, C), generator=gen).to(BF16)
        bias = torch.randn(C, generator=gen) * 0.5
    g = torch.randn((B, H // 2, W // 2, C), generator=gen).to(BF16)
    return PoolOperands(x, bias if with_bias else None, g)


class PoolOut(NamedTuple):
    y: torch.Tensor              # [B][H/2][W/2][C] bf16
    idx: torch.Tensor            # [B][H/2][W/2][C] uint8
    gx: torch.Tensor             # [B][H][W][C] bf16


def pool_restate(op, mut=()):
    """The kernels' rule, straight-line.  Mutants: last_winner (>= for >), dead_passes (a dead window keeps its winner's
    index, so its gradient passes), bias_after_max (the bias joins after both maxima, the pool's and the ReLU's with 0:
    winner and dead windows are decided on x alone; adding it between the two maxima is no mutant, since an fp32 add of
    one value to all four candidates is monotone and the maximum commutes with it)."""
    t = op.x.float()
    late = "bias_after_max" in mut and op.bias is not None
    if op.bias is not None and not late:
        t = t + op.bias
    cand = [t[:, dh::2, dw::2] for dh in (0, 1) for dw in (0, 1)]
    best, idx = cand[0], torch.zeros(cand[0].shape, dtype=torch.uint8)
    for k in (1, 2, 3):
        gt = cand[k] >= best if "last_winner" in mut else cand[k] > best
        best, idx = torch.where(gt, cand[k], best), torch.where(gt, torch.full_like(idx, k), idx)
    dead = best <= 0
    y = torch.where(dead, torch.zeros(()), best)
    y = (y + op.bias if late else y).to(BF16)
    if "dead_passes" not in mut:
        idx = torch.where(dead, torch.full_like(idx, 4), idx)
    gx = torch.zeros(op.x.shape, dtype=BF16)
    for k, (dh, dw) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        gx[:, dh::2, dw::2] = torch.where(idx == k, op.g, torch.zeros((), dtype=BF16))
    return PoolOut(y, idx, gx)


class PoolRow(NamedTuple):
    ops: PoolOperands
    y: torch.Tensor              # torch's chain rounded to bf16
    gx: torch.Tensor             # torch's autograd, fp32 [B][H][W][C]
    live_tied: float             # fraction of windows that are live with a tied maximum
    dead: float                  # fraction of dead windows


@functools.lru_cache(maxsize=None)
def pool_reference(row, with_bias, leg):
    """Operands and torch's own fp32 chain + autograd (CPU) of one pool row, computed once and shared; never modified."""
    B, H, W, C = row
    op = pool_operands(pool_name(B, H, W, C, with_bias), leg, B, H, W, C, with_bias)
    x = op.x.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    t = x if op.bias is None else x + op.bias.view(1, C, 1, 1)
    y = F.max_pool2d(F.relu(t), 2)
    (gx,) = torch.autograd.grad(y, x, op.g.float().permute(0, 3, 1, 2))
    win = F.unfold(t.detach(), 2, stride=2).reshape(B, C, 4, -1)
    top = win.max(2).values
    tied = ((win == top[:, :, None]).sum(2) > 1) & (top > 0)
    return PoolRow(op, y.detach().permute(0, 2, 3, 1).to(BF16).contiguous(), gx.permute(0, 2, 3, 1).contiguous(),
                   float(tied.double().mean()), float((top <= 0).double().mean()))


def same_bits(a, b):
    """Two tensors of bf16-representable (or uint8) values, bit for bit: the sign of a zero counts."""
    if a.dtype == torch.uint8 or b.dtype == torch.uint8:
        return a.shape == b.shape and torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.float().contiguous().view(torch.int32), b.float().contiguous().view(torch.int32))
