"""Row table, operand generators and packers of the 32-channel 3x3 convolution kernels (adil_dense3x3_fwd /
adil_dense3x3_bwd, csrc/adil_dense3x3.hip).  The fp64 restatement, the two legs and the comparators are those of
tests/classifier_reference.py (`conv3x3`, `conv3x3_bwd`, `compare_exact`, `assert_premise`, `gaussian_ratio`); nothing of
them is restated here.

exact leg     x, g integers in [-16, 16], w integers in [-8, 8]: every product and partial sum is an integer below
              9 * 512 * 16 * 8 < 2^20, exact in fp32 in any order; the outputs are compared bit for bit.
gaussian leg  x, g ~ N(0, 1), w ~ N(0, 1 / (9 R)) with R the reduction of the direction the weight is used in (the forward's
              C; the gradient gets a weight of its own with fan-in 9 N), bound gaussian_ratio <= 1."""
import functools
from typing import NamedTuple

import torch

from classifier_reference import (Arith, Gen, Out, _taps_linear, assert_premise, compare_exact, conv3x3, conv3x3_bwd,  # noqa: F401
                                  finish, gaussian_ratio, pack_taps, pack_taps_flipped, stats)

TILE = 256                       # pixels of a workgroup of d3_kernel

# (B, H, W, C, N): both directions run on every row
NETWORK_ROWS = [(2, 7, 7, 128, 32), (1, 14, 14, 128, 32), (1, 28, 28, 128, 32), (1, 56, 56, 128, 32)]
EDGE_ROWS = [
    (1, 1, 1, 32, 32),           # one pixel
    (3, 6, 10, 64, 32),          # image boundaries inside one tile
    (1, 3, 63, 32, 64),          # the widest halo
    (2, 63, 1, 96, 32),          # W = 1: six of nine taps always masked
    (1, 1, 63, 64, 96),          # H = 1
    (3, 22, 18, 160, 96),        # neither side a multiple of 64; 1188 pixels
    (1, 9, 15, 512, 32),         # the largest reduction forward
    (1, 9, 15, 32, 512),         # the largest reduction backward
    (1, 127, 1, 32, 32),         # 127 pixels
    (2, 8, 8, 32, 32),           # 128 pixels
    (1, 3, 43, 64, 32),          # 129 pixels
    (1, 257, 1, 32, 32),         # one pixel more than a 256-pixel tile
    (1, 15, 17, 32, 32),         # 255 pixels: tile - 1
    (1, 16, 16, 32, 32),         # 256 pixels: the tile
    (1, 33, 63, 32, 96),         # 2079 pixels = nine pixel tiles, eight of them dealt round-robin to the XCDs with their
    (1, 33, 63, 96, 32),         # three channel tiles of 32, forward (N = 96) and gradient (C = 96)
]
ROWS = NETWORK_ROWS + EDGE_ROWS
NAN_ROWS = [(3, 6, 10, 64, 32), (1, 3, 63, 32, 64)]
MASK_ROW = (3, 6, 10, 64, 32)
HASH_ROWS = [(1, 28, 28, 128, 32), (3, 22, 18, 160, 96), (1, 3, 63, 32, 64)]

# (B, H, W, C, N) the entry points refuse: C or N of 16, 48, 544 or 0; W = 0 or 64; H = 0; B = 0 or -1
REFUSED_DIMS = ([(2, 4, 4, c, 32) for c in (16, 48, 544, 0)] + [(2, 4, 4, 32, n) for n in (16, 48, 544, 0)]
                + [(2, 4, 0, 32, 32), (2, 4, 64, 32, 32), (2, 0, 4, 32, 32), (0, 4, 4, 32, 32), (-1, 4, 4, 32, 32)])

# (C, N, H) of the 58 growth convolutions of DenseNet-121 at 224 x 224, in network order
DENSENET_GROWTH_LAYERS = [(128, 32, h) for h, n in ((56, 6), (28, 12), (14, 24), (7, 16)) for _ in range(n)]


def row_name(B, H, W, C, N):
    return "dense3x3/%dx%dx%d/%d->%d" % (B, H, W, C, N)


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
    """The kernel on its packed weights, as an Arith emulation: OUT[m][o] = sum_tap rows_tap(src)[m] . wp[o][tap], taps in
    the kernel's linear pixel shift with its validity mask.  src [B][H][W][R], wp [O][9][R].  `tap_transposed` reads
    tap kw*3 + kh."""
    B, H, W, R = src.shape
    O = wp.shape[0]
    dt = ar.dtype
    acc = torch.zeros(B * H * W, O, dtype=dt)
    for kh, kw, rows in _taps_linear(ar, src.to(dt), H, W):
        tap = kw * 3 + kh if "tap_transposed" in mut else kh * 3 + kw
        acc = acc + ar.mm(rows, wp[:, tap].to(dt).t())
    return finish(ar, Out(acc.reshape(B, H, W, O), None, 9 * R))


def pack_bwd_unflipped(w):
    """The mutant of the gradient pack: channels swapped, taps NOT flipped."""
    return pack_taps(w.transpose(0, 1))
