"""GPU: the 3x3 convolution kernels give, through adil_conv3x3, adil_conv3x3_s2_fwd and adil_conv3x3_s2_bwd, the bits that
the (chunk, tap) step loop they once replaced gave on the same operands (tests/retired_bits.py; the two loops agreed bit
for bit when the record was taken): gaussian bf16 operands with NaN in the memory around every input, canaries around every
output, on shapes that reach the partial tile, the width limit, several channel chunks (the halo reload and the register
rotation across chunk boundaries), both tile shapes and both workgroup maps; and under graph capture."""
import pytest
import torch

import retired_bits as RB

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAD = 4096                                          # elements of guard on each side (a multiple of 8: 16-byte alignment stays)
CANARY = 7.0


def _lib():
    from dl_attack_on_imagenet_amd import _lib as L
    return L.load()


def _ops():
    from dl_attack_on_imagenet_amd import ops
    return ops


def _guarded(t):
    """A copy of the bf16 tensor `t` on the device with PAD elements of NaN in front of and behind it."""
    buf = torch.full((t.numel() + 2 * PAD,), float("nan"), dtype=torch.bfloat16, device=DEV)
    buf[PAD:PAD + t.numel()] = t.reshape(-1).to(DEV)
    return buf, buf[PAD:PAD + t.numel()].view(t.shape)


def _out(rows, cols):
    buf = torch.full((rows * cols + 2 * PAD,), CANARY, dtype=torch.bfloat16, device=DEV)
    return buf, buf[PAD:PAD + rows * cols].view(rows, cols)


def _check(case, inputs, res):
    buf, y = res
    torch.cuda.synchronize()
    assert bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all()), case
    assert bool(torch.isfinite(y.float()).all()), case                  # no NaN from around the inputs
    assert float(y.float().abs().sum()) > 0, case                       # not a vacuous comparison
    assert not bool((y == CANARY).all(dim=1).any()), case               # every row written
    RB.check(case, inputs, y)


def _weights(n, c, gen):
    return (torch.randn(n, c, 3, 3, generator=gen) / (9 * c) ** 0.5).bfloat16()


# (B, H, W, C, N, flipped): see the module docstring; M = 70 (one partial tile, image smaller than the halo), 189 at W = 63
# with three chunks, 1960 with NT = 3 and MT = 16 (the swizzled map), 504 at W = 56 (MT = 4: plain map, N = 64 -> the
# 256-pixel tile), a column, eight chunks, N = 256, and two of them as the input gradient (C <-> N on the flipped pack)
S1 = [(2, 5, 7, 64, 64, False), (3, 1, 63, 192, 64, False), (40, 7, 7, 64, 192, False), (1, 9, 56, 64, 64, False),
      (3, 30, 1, 64, 128, False), (2, 3, 2, 512, 128, False), (20, 7, 7, 128, 256, False), (2, 4, 63, 64, 128, False),
      (3, 1, 63, 192, 64, True), (20, 7, 7, 128, 256, True)]


def s1_case(b, h, w_, c, n, flipped):
    """(case id, inputs in the digest's order, call): call() runs adil_conv3x3 into a fresh guarded output, call(res) into
    the guarded output `res`."""
    lib, o = _lib(), _ops()
    gen = torch.Generator().manual_seed(b * h * w_ + c + 3 * n + int(flipped))
    wf, wb = o.pack_conv3x3_weights(_weights(n, c, gen).to(DEV))
    cin, cout, pack = (n, c, wb) if flipped else (c, n, wf)              # the gradient: g [.., N] -> gx [.., C] on wp' [C][9][N]
    assert pack.shape == (cout, 9 * cin)
    _, x = _guarded(torch.randn(b, h, w_, cin, generator=gen).bfloat16())
    _, wp = _guarded(pack)
    m = b * h * w_

    def call(res=None):
        buf, y = res or _out(m, cout)
        assert lib.adil_conv3x3(o._ptr(x), o._ptr(wp), o._ptr(y), b, h, w_, cin, cout, o._stream()) == 0
        return buf, y

    return f"conv3x3 {b}x{h}x{w_} C{c} N{n}{' flipped' if flipped else ''}", [x, wp], call


@pytest.mark.parametrize("b,h,w_,c,n,flipped", S1)
def test_stride1_gives_the_recorded_bits(b, h, w_, c, n, flipped):
    case, inputs, call = s1_case(b, h, w_, c, n, flipped)
    _check(case, inputs, call())


S2 = [(3, 2, 2, 64, 64), (2, 6, 62, 128, 192), (19, 14, 14, 64, 256), (5, 2, 62, 256, 128), (1, 8, 2, 64, 128)]


def s2_cases(b, h, w_, c, n):
    """The forward and the gradient of one row, each as s1_case gives them."""
    lib, o = _lib(), _ops()
    gen = torch.Generator().manual_seed(b * h * w_ + c + 3 * n)
    wf, wb = o.pack_conv3x3_s2_weights(_weights(n, c, gen).to(DEV))
    _, x = _guarded(torch.randn(b, h, w_, c, generator=gen).bfloat16())
    _, g = _guarded(torch.randn(b, h // 2, w_ // 2, n, generator=gen).bfloat16())
    _, wpf = _guarded(wf)
    _, wpb = _guarded(wb)
    m4 = b * h * w_

    def fwd(res=None):
        buf, y = res or _out(m4 // 4, n)
        assert lib.adil_conv3x3_s2_fwd(o._ptr(x), o._ptr(wpf), o._ptr(y), b, h, w_, c, n, o._stream()) == 0
        return buf, y

    def bwd(res=None):
        buf, gx = res or _out(m4, c)
        assert lib.adil_conv3x3_s2_bwd(o._ptr(g), o._ptr(wpb), o._ptr(gx), b, h, w_, c, n, o._stream()) == 0
        return buf, gx

    row = f"{b}x{h}x{w_} C{c} N{n}"
    return [(f"conv3x3_s2 fwd {row}", [x, wpf], fwd), (f"conv3x3_s2 bwd {row}", [g, wpb], bwd)]


@pytest.mark.parametrize("b,h,w_,c,n", S2)
def test_stride2_forward_and_gradient_give_the_recorded_bits(b, h, w_, c, n):
    for case, inputs, call in s2_cases(b, h, w_, c, n):
        _check(case, inputs, call())


def test_graph_replay_gives_the_recorded_bits():
    """One call captured, its output refilled with canaries, replayed: the replay gives the recorded bits and leaves the
    guards alone."""
    case, inputs, call = s1_case(2, 4, 63, 64, 128, False)
    call()                                                               # warms the kernel up outside the capture
    torch.cuda.synchronize()
    buf, y = _out(2 * 4 * 63, 128)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call((buf, y))
    buf.fill_(CANARY)
    graph.replay()
    _check(case, inputs, (buf, y))
    del graph
