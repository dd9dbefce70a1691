"""GPU: the wide output tiles of the pointwise forward (pw_conv_fwd_kernel<256 / 512, ., ., 8 waves>, reached through
adil_pw_conv_fwd_tile(..., bn=256 / 512)) are bitwise the narrow tile (bn=128) on every argument of the ABI — the residual,
relu 0/1, the BatchNorm + ReLU prologue, the stride-2 gather, ragged M, the XCD swizzle branch — and write nothing past
their output; a forced tile that does not cover the call is refused; adil_pw_conv_fwd follows adil_pw_route_policy."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
WIDE = (256, 512)                               # the wide tiles the library keeps
CANARY = 7.0


def _lib():
    from dl_attack_on_imagenet_amd import _lib as L
    return L.load()


def _ops():
    from dl_attack_on_imagenet_amd import ops
    return ops


def _operands(rows, m, k, n, seed):
    """rows = pixels of x (m, or the 4 m of the stride-2 input grid).  Unit normal bf16 activations, weights scaled by
    fan-in ** -0.5, BatchNorm tables in [0.5, 1.5) and N(0, 0.3), as tests/test_gpu_pw_wide.py builds them."""
    gen = torch.Generator().manual_seed(seed)
    bf = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).bfloat16().to(DEV)
    return dict(x=bf(rows, k), w=bf(n, k, sc=k ** -0.5), res=bf(m, n),
                scale=(0.5 + torch.rand(n, generator=gen)).to(DEV), shift=(torch.randn(n, generator=gen) * 0.3).to(DEV),
                ps=(0.5 + torch.rand(k, generator=gen)).to(DEV), pb=(torch.randn(k, generator=gen) * 0.3).to(DEV))


def _call(lib, o, t, m, k, n, res, relu, pro, sub_w, sub_hw, bn):
    """bn = None: adil_pw_conv_fwd (the routed call).  Returns rc and y with one canary row behind it."""
    p = o._ptr
    y = torch.full((m + 1, n), CANARY, dtype=torch.bfloat16, device=DEV)
    args = (p(t["x"]), p(t["w"]), p(t["scale"]), p(t["shift"]), p(t["res"]) if res else None, p(y), m, k, n, relu,
            p(t["ps"]) if pro else None, p(t["pb"]) if pro else None, sub_w, sub_hw, o._stream())
    rc = lib.adil_pw_conv_fwd(*args) if bn is None else lib.adil_pw_conv_fwd_tile(*args, bn)
    torch.cuda.synchronize()
    return rc, y


def _same(y_a, y_b, m, what):
    assert torch.equal(y_b[:m].view(torch.int16), y_a[:m].view(torch.int16)), what
    assert bool((y_b[m:] == CANARY).all()) and bool((y_a[m:] == CANARY).all()), what
    assert float(y_a[:m].float().abs().sum()) > 0, what                      # not a vacuous comparison


# M: 98 < one tile; 333 ragged; 1024 -> MT = 8 (the XCD swizzle branch); 1029 -> MT = 9 (plain map)
@pytest.mark.parametrize("k,n", [(256, 1024), (512, 2048), (1024, 256), (64, 256)])
@pytest.mark.parametrize("m", [98, 333, 1024, 1029])
def test_wide_tile_is_bitwise_the_narrow_tile(m, k, n):
    lib, o = _lib(), _ops()
    t = _operands(m, m, k, n, 7 * m + n + k)
    pros = (False, True) if k <= 512 else (False,)
    for res, relu, pro in itertools.product((False, True), (0, 1), pros):
        rc, y_a = _call(lib, o, t, m, k, n, res, relu, pro, 0, 0, 128)
        assert rc == 0
        for bn in (b for b in WIDE if n % b == 0):
            rc, y_b = _call(lib, o, t, m, k, n, res, relu, pro, 0, 0, bn)
            assert rc == 0
            _same(y_a, y_b, m, (bn, res, relu, pro))


# (images, OH, OW, K, N): 19 x 7 x 7 -> M = 931, ragged, MT = 8; 1 x 7 x 11 -> M = 77, one partial tile
@pytest.mark.parametrize("b,oh,ow,k,n", [(19, 7, 7, 128, 256), (1, 7, 11, 1024, 2048)])
def test_wide_tile_gathers_the_stride_2_pixels(b, oh, ow, k, n):
    lib, o = _lib(), _ops()
    m = b * oh * ow
    t = _operands(4 * m, m, k, n, m + k + n)
    pros = (False, True) if k <= 512 else (False,)
    for pro in pros:
        rc, y_a = _call(lib, o, t, m, k, n, False, 0, pro, ow, oh * ow, 128)
        assert rc == 0
        # the narrow tile itself against the gathered rows through the stride-1 form (the wide comparison is not blind
        # to a gather both tiles get wrong in the same way)
        xg = t["x"].view(b, 2 * oh, 2 * ow, k)[:, ::2, ::2].reshape(m, k).contiguous()
        rc, y_g = _call(lib, o, dict(t, x=xg), m, k, n, False, 0, pro, 0, 0, 128)
        assert rc == 0
        _same(y_g, y_a, m, ("gathered rows", pro))
        for bn in (w for w in WIDE if n % w == 0):
            rc, y_b = _call(lib, o, t, m, k, n, False, 0, pro, ow, oh * ow, bn)
            assert rc == 0
            _same(y_a, y_b, m, (bn, pro))


def test_forced_tile_is_refused_where_it_does_not_cover():
    lib, o = _lib(), _ops()
    m, k, n = 200, 128, 256
    t = _operands(m, m, k, n, 1)
    for bn in (96, 512):                                                     # no tile at all; N % 512 != 0
        rc, y = _call(lib, o, t, m, k, n, True, 1, True, 0, 0, bn)
        assert rc == -1 and bool((y == CANARY).all()), bn
    rc, y = _call(lib, o, t, m, k, n, True, 1, True, 0, 0, 256)              # the same call at a tile that covers it runs
    assert rc == 0 and float(y[:m].float().abs().sum()) > 0 and bool((y[m:] == CANARY).all())


def test_forward_follows_the_route_policy():
    lib, o = _lib(), _ops()
    m, k, n = 333, 256, 1024
    t = _operands(m, m, k, n, 2)
    prev = lib.adil_pw_route_policy(-1)
    try:
        forced = {bn: _call(lib, o, t, m, k, n, True, 1, True, 0, 0, bn)[1] for bn in (128, 512)}
        lib.adil_pw_route_policy(1)
        rc, y1 = _call(lib, o, t, m, k, n, True, 1, True, 0, 0, None)
        assert rc == 0
        lib.adil_pw_route_policy(2)
        rc, y2 = _call(lib, o, t, m, k, n, True, 1, True, 0, 0, None)
        assert rc == 0
    finally:
        lib.adil_pw_route_policy(prev)
    _same(forced[128], y1, m, "policy 1")
    _same(forced[512], y2, m, "policy 2")
