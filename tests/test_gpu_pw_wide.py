"""GPU: the wide output tiles of the pointwise input gradient (pw_conv_bwd_kernel<256 / 512, G3=0, 8 waves>, reached through
adil_pw_conv_bwd_tile(..., bo=256 / 512)) are bitwise the parent tile (bo=128) on every argument of the ABI it covers — g2, gres,
relu 0/1, the xin epilogue, ragged M, the XCD swizzle branch — and writes nothing past its outputs; the forced tile is
refused where it does not cover the call; FusedResNet-50 gives the same bits with the wide tile everywhere
(adil_pw_route_policy(2)) as with the parent's tiles everywhere (policy 1)."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
WIDE = (256, 512)                               # the wide tiles the library keeps


def _lib():
    from dl_attack_on_imagenet_amd import _lib as L
    return L.load()


def _ops():
    from dl_attack_on_imagenet_amd import ops
    return ops


def _operands(m, n, k, seed):
    """As tests/test_gpu_pw_join.py builds them: unit normal bf16 gradients, y and xin as a forward would leave them,
    weights scaled by fan-in ** -0.5, BatchNorm tables in [0.5, 1.5) and N(0, 0.3)."""
    gen = torch.Generator().manual_seed(seed)
    bf = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).bfloat16().to(DEV)
    return dict(g=bf(m, n), g2=bf(m, n), y=torch.relu(bf(m, n)), wt=bf(k, n, sc=n ** -0.5), xin=bf(m, k),
                scale=(0.5 + torch.rand(n, generator=gen)).to(DEV),
                ps=(0.5 + torch.rand(k, generator=gen)).to(DEV), pb=(torch.randn(k, generator=gen) * 0.3).to(DEV))


def _run(lib, o, t, m, n, k, bo, g2, gres, relu, xin):
    p = o._ptr
    gx = torch.full((m + 1, k), 7.0, dtype=torch.bfloat16, device=DEV)          # one canary row behind each output
    gr = torch.full((m + 1, n), 7.0, dtype=torch.bfloat16, device=DEV)
    rc = lib.adil_pw_conv_bwd_tile(p(t["g"]), p(t["g2"]) if g2 else None, p(t["y"]), p(t["scale"]), p(t["wt"]), p(gx),
                                   p(gr) if gres else None, m, k, n, relu, p(t["xin"]) if xin else None,
                                   p(t["ps"]) if xin else None, p(t["pb"]) if xin else None, None, 0, 0, o._stream(), bo)
    return rc, gx, gr


# M: 98 < one tile; 333 ragged; 1024 -> MT = 8 (the XCD swizzle branch); 1029 -> MT = 9 (plain map)
@pytest.mark.parametrize("n,k", [(1024, 256), (2048, 512), (256, 1024), (64, 256)])
@pytest.mark.parametrize("m", [98, 333, 1024, 1029])
def test_wide_tile_is_bitwise_the_parent_tile(m, n, k):
    lib, o = _lib(), _ops()
    t = _operands(m, n, k, 7 * m + n + k)
    xins = (False, True) if k <= 512 else (False,)
    for g2, gres, relu, xin in itertools.product((False, True), (False, True), (0, 1), xins):
        rc, gx_a, gr_a = _run(lib, o, t, m, n, k, 128, g2, gres, relu, xin)
        assert rc == 0
        for bo in (b for b in WIDE if k % b == 0):
            rc, gx_b, gr_b = _run(lib, o, t, m, n, k, bo, g2, gres, relu, xin)
            assert rc == 0
            torch.cuda.synchronize()
            what = (bo, g2, gres, relu, xin)
            assert torch.equal(gx_b[:m].view(torch.int16), gx_a[:m].view(torch.int16)), what
            assert bool((gx_b[m:] == 7.0).all()) and bool((gx_a[m:] == 7.0).all()), what
            if gres:
                assert torch.equal(gr_b[:m].view(torch.int16), gr_a[:m].view(torch.int16)), what
                assert bool((gr_b[m:] == 7.0).all()), what
            else:
                assert bool((gr_b == 7.0).all()), what                       # no gres pointer: nothing written
            assert float(gx_a[:m].float().abs().sum()) > 0, what             # not a vacuous comparison


def test_forced_wide_tile_is_refused_where_it_does_not_cover():
    lib, o = _lib(), _ops()
    p = o._ptr
    m = 256                                                                  # 4 images of 8 x 8 for the g3 case
    for bo in WIDE:
        t = _operands(m, 128, 128, 1)                                        # K % 256 != 0
        rc, gx, gr = _run(lib, o, t, m, 128, 128, bo, True, True, 1, False)
        torch.cuda.synchronize()
        assert rc == -1 and bool((gx == 7.0).all()) and bool((gr == 7.0).all())
        t = _operands(m, 64, 512, 2)                                         # g3 set (K = 512: either tile would cover it)
        g3 = torch.zeros(m // 4, 64, dtype=torch.bfloat16, device=DEV)
        gx = torch.full((m + 1, 512), 7.0, dtype=torch.bfloat16, device=DEV)
        gr = torch.full((m + 1, 64), 7.0, dtype=torch.bfloat16, device=DEV)
        args = (p(t["g"]), None, p(t["y"]), p(t["scale"]), p(t["wt"]), p(gx), p(gr), m, 512, 64, 1, None, None, None, p(g3),
                4, 16, o._stream())
        assert lib.adil_pw_conv_bwd_tile(*args, bo) == -1
        torch.cuda.synchronize()
        assert bool((gx == 7.0).all()) and bool((gr == 7.0).all())
        assert lib.adil_pw_conv_bwd_tile(*args, 128) == 0                    # the same call at the parent tile runs
        torch.cuda.synchronize()
        assert float(gx[:m].float().abs().sum()) > 0 and bool((gx[m:] == 7.0).all())
    t = _operands(m, 64, 256, 3)
    assert _run(lib, o, t, m, 64, 256, 96, False, False, 1, False)[0] == -1  # not a tile at all


def test_route_policy_returns_the_previous_value():
    lib = _lib()
    first = lib.adil_pw_route_policy(1)
    try:
        assert lib.adil_pw_route_policy(2) == 1
        assert lib.adil_pw_route_policy(7) == 2 and lib.adil_pw_route_policy(-1) == 2      # out of range: a query
    finally:
        lib.adil_pw_route_policy(first)
    assert first == 0 and lib.adil_pw_route_policy(-1) == 0                  # the default is the table


def test_fused_resnet50_is_bitwise_the_same_under_either_policy():
    """own_strided_conv=True: no library convolution in the network, so it is reproducible call to call."""
    from dl_attack_on_imagenet_amd import zoo
    lib = _lib()
    model = zoo.build_classifier("resnet50", num_classes=10, seed=5, device=DEV, dtype=torch.bfloat16, channels_last=True,
                                 fuse_bn_act=True, fuse_stem=True, own_strided_conv=True)
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(0)).to(DEV).bfloat16()
    prev = lib.adil_pw_route_policy(-1)
    out = {}
    try:
        for policy in (1, 2):
            lib.adil_pw_route_policy(policy)
            xi = x.clone().requires_grad_(True)
            lo = model(xi)
            (g,) = torch.autograd.grad(lo.float().square().sum(), xi)
            torch.cuda.synchronize()
            out[policy] = (lo.detach().clone(), g.clone())
    finally:
        lib.adil_pw_route_policy(prev)
    assert torch.equal(out[1][0].view(torch.int16), out[2][0].view(torch.int16))
    assert torch.equal(out[1][1].view(torch.int16), out[2][1].view(torch.int16))
    assert float(out[1][1].float().abs().sum()) > 0
