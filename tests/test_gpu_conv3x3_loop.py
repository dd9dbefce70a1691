"""GPU: the two main loops of the 3x3 convolution kernels (adil_conv3x3_loop: 0 = unrolled taps and pipelined LDS reads,
1 = the step loop it replaced) give the same bits through adil_conv3x3, adil_conv3x3_s2_fwd and adil_conv3x3_s2_bwd:
gaussian bf16 operands with NaN in the memory around every input, canaries around every output, on shapes that reach the
partial tile, the width limit, several channel chunks (the halo reload and the register rotation across chunk
boundaries), both tile shapes and both workgroup maps; under graph capture; and the switch's own contract."""
import pytest
import torch

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


def _check_pair(res, what):
    (buf0, y0), (buf1, y1) = res[0], res[1]
    torch.cuda.synchronize()
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16)), what
    for buf in (buf0, buf1):
        assert bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all()), what
    assert bool(torch.isfinite(y0.float()).all()), what                 # no NaN from around the inputs
    assert float(y0.float().abs().sum()) > 0, what                      # not a vacuous comparison
    assert not bool((y0 == CANARY).all(dim=1).any()), what              # every row written


def _both_loops(lib, call):
    prev = lib.adil_conv3x3_loop(-1)
    res = {}
    try:
        for variant in (1, 0):
            assert lib.adil_conv3x3_loop(variant) in (0, 1)
            res[variant] = call()
    finally:
        lib.adil_conv3x3_loop(prev)
    return res


def _weights(n, c, gen):
    return (torch.randn(n, c, 3, 3, generator=gen) / (9 * c) ** 0.5).bfloat16()


# (B, H, W, C, N, flipped): see the module docstring; M = 70 (one partial tile, image smaller than the halo), 189 at W = 63
# with three chunks, 1960 with NT = 3 and MT = 16 (the swizzled map), 504 at W = 56 (MT = 4: plain map, N = 64 -> the
# 256-pixel tile), a column, eight chunks, N = 256, and two of them as the input gradient (C <-> N on the flipped pack)
S1 = [(2, 5, 7, 64, 64, False), (3, 1, 63, 192, 64, False), (40, 7, 7, 64, 192, False), (1, 9, 56, 64, 64, False),
      (3, 30, 1, 64, 128, False), (2, 3, 2, 512, 128, False), (20, 7, 7, 128, 256, False), (2, 4, 63, 64, 128, False),
      (3, 1, 63, 192, 64, True), (20, 7, 7, 128, 256, True)]


@pytest.mark.parametrize("b,h,w_,c,n,flipped", S1)
def test_stride1_new_loop_is_bitwise_the_parent_loop(b, h, w_, c, n, flipped):
    lib, o = _lib(), _ops()
    gen = torch.Generator().manual_seed(b * h * w_ + c + 3 * n + int(flipped))
    wf, wb = o.pack_conv3x3_weights(_weights(n, c, gen).to(DEV))
    cin, cout, pack = (n, c, wb) if flipped else (c, n, wf)              # the gradient: g [.., N] -> gx [.., C] on wp' [C][9][N]
    assert pack.shape == (cout, 9 * cin)
    _, x = _guarded(torch.randn(b, h, w_, cin, generator=gen).bfloat16())
    _, wp = _guarded(pack)
    m = b * h * w_

    def call():
        buf, y = _out(m, cout)
        assert lib.adil_conv3x3(o._ptr(x), o._ptr(wp), o._ptr(y), b, h, w_, cin, cout, o._stream()) == 0
        return buf, y

    _check_pair(_both_loops(lib, call), (b, h, w_, c, n, flipped))


S2 = [(3, 2, 2, 64, 64), (2, 6, 62, 128, 192), (19, 14, 14, 64, 256), (5, 2, 62, 256, 128), (1, 8, 2, 64, 128)]


@pytest.mark.parametrize("b,h,w_,c,n", S2)
def test_stride2_forward_and_gradient_are_bitwise_the_same_under_either_loop(b, h, w_, c, n):
    lib, o = _lib(), _ops()
    gen = torch.Generator().manual_seed(b * h * w_ + c + 3 * n)
    wf, wb = o.pack_conv3x3_s2_weights(_weights(n, c, gen).to(DEV))
    _, x = _guarded(torch.randn(b, h, w_, c, generator=gen).bfloat16())
    _, g = _guarded(torch.randn(b, h // 2, w_ // 2, n, generator=gen).bfloat16())
    _, wpf = _guarded(wf)
    _, wpb = _guarded(wb)
    m4 = b * h * w_

    def fwd():
        buf, y = _out(m4 // 4, n)
        assert lib.adil_conv3x3_s2_fwd(o._ptr(x), o._ptr(wpf), o._ptr(y), b, h, w_, c, n, o._stream()) == 0
        return buf, y

    def bwd():
        buf, gx = _out(m4, c)
        assert lib.adil_conv3x3_s2_bwd(o._ptr(g), o._ptr(wpb), o._ptr(gx), b, h, w_, c, n, o._stream()) == 0
        return buf, gx

    _check_pair(_both_loops(lib, fwd), ("fwd", b, h, w_, c, n))
    _check_pair(_both_loops(lib, bwd), ("bwd", b, h, w_, c, n))


def test_graph_capture_keeps_the_variant_in_force_at_capture():
    """One call captured under each variant, replayed with the OTHER variant in force: the replay launches what was
    captured (the switch is a host-side int read at launch, and a replay launches nothing through the host entry), the
    bits are those of an eager call, and the replay leaves the switch alone."""
    lib, o = _lib(), _ops()
    b, h, w_, c, n = 2, 4, 63, 64, 128
    gen = torch.Generator().manual_seed(11)
    wf, _ = o.pack_conv3x3_weights(_weights(n, c, gen).to(DEV))
    _, x = _guarded(torch.randn(b, h, w_, c, generator=gen).bfloat16())
    _, wp = _guarded(wf)
    m = b * h * w_
    prev = lib.adil_conv3x3_loop(-1)
    try:
        lib.adil_conv3x3_loop(1)
        _, ref = _out(m, n)
        assert lib.adil_conv3x3(o._ptr(x), o._ptr(wp), o._ptr(ref), b, h, w_, c, n, o._stream()) == 0   # also warms both up
        lib.adil_conv3x3_loop(0)
        _, warm = _out(m, n)
        assert lib.adil_conv3x3(o._ptr(x), o._ptr(wp), o._ptr(warm), b, h, w_, c, n, o._stream()) == 0
        torch.cuda.synchronize()
        for variant in (0, 1):
            lib.adil_conv3x3_loop(variant)
            buf, y = _out(m, n)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                assert lib.adil_conv3x3(o._ptr(x), o._ptr(wp), o._ptr(y), b, h, w_, c, n, o._stream()) == 0
            assert lib.adil_conv3x3_loop(1 - variant) == variant
            buf.fill_(CANARY)
            graph.replay()
            torch.cuda.synchronize()
            assert lib.adil_conv3x3_loop(-1) == 1 - variant
            assert torch.equal(y.view(torch.int16), ref.view(torch.int16)), variant
            assert bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all()), variant
            del graph
    finally:
        lib.adil_conv3x3_loop(prev)


def test_switch_returns_the_previous_value_and_ignores_other_arguments():
    lib = _lib()
    first = lib.adil_conv3x3_loop(1)
    try:
        assert lib.adil_conv3x3_loop(0) == 1
        assert lib.adil_conv3x3_loop(1) == 0
        assert lib.adil_conv3x3_loop(2) == 1 and lib.adil_conv3x3_loop(-1) == 1 and lib.adil_conv3x3_loop(9) == 1
    finally:
        lib.adil_conv3x3_loop(first)
    assert first == 0 and lib.adil_conv3x3_loop(-1) == 0                 # the default is the new loop
