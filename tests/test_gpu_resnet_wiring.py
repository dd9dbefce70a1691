"""What stands between the classifier kernels and the attack: ops.PointwiseConvFunction / PointwiseJoinFunction /
Conv3x3Function / AffineActFunction and the block logic of zoo._ConvAffine, zoo._FusedResBlock and zoo.FusedResNet.

(a) each function against single calls of the C ABI, bit for bit, option by option;
(b) FusedResNet on two small networks against the straight-line tape of tests/resnet_tape.py run on the C ABI: every
    block output, the last output and the gradient with respect to the pooled stem output, bit for bit;
(c) every step of such a tape run against its fp64 restatement on the step's actual inputs, within the derived
    element-wise bound of classifier_reference (ratio <= 1), at the composite shapes M = 1152, 288, 72, 18;
(d) two mutants of PointwiseConvFunction.backward that only omit an optional pointer (g_sub, g_twin): (b) must report them.

The tape itself is held to the fp64 torch modules by tests/test_resnet_wiring_cpu.py.  profiles/resnet_wiring.md has the
measured values."""
import time

import pytest
import torch
import torch.nn.functional as F

import classifier_reference as R
import resnet_tape as T
from classifier_reference import BF16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ops():
    from dl_attack_on_imagenet_amd import ops as o
    return o


def lib():
    from dl_attack_on_imagenet_amd import _lib
    return _lib.load()


def abi(**kw):
    return T.Abi(lib(), **kw)


def same(a, b):
    """bf16 tensors of one logical shape hold the same bits."""
    return a.shape == b.shape and a.dtype == b.dtype == BF16 and torch.equal(R.bits(a), R.bits(b))


def nchw(rows, b, h, w):
    """[M][C] rows or an NHWC tensor as the NCHW-shaped channels_last view the functions take."""
    return rows.reshape(b, h, w, -1).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


class Layer:
    """Seeded operands of one pointwise layer K -> N on a b x h x w grid, on the device."""

    def __init__(self, name, b, h, w, K, N):
        G = R.Gen("wiring/" + name, "gaussian")
        self.b, self.h, self.w, self.K, self.N, self.M = b, h, w, K, N, b * h * w
        d = lambda t: t.to(DEV).contiguous()
        self.x, self.res = d(G.act(self.M, K)), d(G.act(self.M, N))
        self.w2d = d(G.weight(N, K))
        self.wt2d = d(self.w2d.t())
        self.scale, self.shift, self.pscale, self.pshift = d(G.scale(N)), d(G.shift(N)), d(G.scale(K)), d(G.shift(K))
        self.g, self.g2, self.g3 = d(G.act(self.M, N)), d(G.act(self.M, N)), d(G.act(self.M // 4, N))
        self.G = G


# ------------------------------------------------------------------------------------------ (a) pointwise, forward
@pytest.mark.parametrize("outputs", [1, 2, 3])
@pytest.mark.parametrize("res,relu,pre", [(r, a, q) for r in (False, True) for a in (False, True) for q in (False, True)])
def test_pointwise_forward_equals_the_c_abi_bitwise(outputs, res, relu, pre):
    o, b, h, w = ops(), 2, 12, 10
    L = Layer("fwd", b, h, w, 64, 128)
    x = nchw(L.x, b, h, w)
    assert x.is_contiguous(memory_format=torch.channels_last)
    want = abi().step("pw_fwd", x=L.x, w=L.w2d, scale=L.scale, shift=L.shift, res=L.res if res else None, relu=int(relu),
                      pscale=L.pscale if pre else None, pshift=L.pshift if pre else None)["y"]
    got = o.pointwise_conv_affine(x, L.w2d, L.wt2d, L.scale, L.shift, res=nchw(L.res, b, h, w) if res else None, relu=relu,
                                  outputs=outputs, pre=(L.pscale, L.pshift) if pre else None)
    got = (got,) if outputs == 1 else got
    assert len(got) == outputs
    y = got[0]
    assert y.shape == (b, 128, h, w) and nhwc(y).is_contiguous() and same(nhwc(y).reshape(-1, 128), want)
    if outputs >= 2:
        assert got[1].data_ptr() == y.data_ptr() and got[1].shape == y.shape and got[1].stride() == y.stride()
    if outputs == 3:
        s = got[2]
        assert s.data_ptr() == y.data_ptr() and s.shape == (b, 128, h // 2, w // 2)
        assert tuple(s.stride()) == (h * w * 128, 1, 2 * w * 128, 2 * 128) and torch.equal(s, y[:, :, ::2, ::2])


@pytest.mark.parametrize("in_place", [True, False])
def test_pointwise_stride2_reads_a_view_in_place_or_copies(in_place):
    """stride2 on a true [:, :, ::2, ::2] view of a channels_last tensor is gathered in place (sub_w = OW); a view whose
    strides do not match (here: of an NCHW-contiguous tensor) is copied; both give the bits of the C ABI's gather."""
    o, b, h, w = ops(), 3, 12, 10
    L = Layer("s2", b, h, w, 64, 128)
    oh, ow = h // 2, w // 2
    want = abi().step("pw_fwd", x=L.x, w=L.w2d, scale=L.scale, shift=L.shift, res=None, relu=0, sub_w=ow, sub_hw=oh * ow,
                      M=b * oh * ow)["y"]
    full = nchw(L.x, b, h, w) if in_place else nchw(L.x, b, h, w).contiguous()
    view = full[:, :, ::2, ::2]
    pattern = (4 * oh * ow * 64, 1, 4 * ow * 64, 2 * 64)
    assert (tuple(view.stride()) == pattern) == in_place and view.data_ptr() == full.data_ptr()
    seen = []
    loaded = lib()

    class Spy:                                                         # the library with one entry point observed
        def __getattr__(self, name):
            fn = getattr(loaded, name)
            if name != "adil_pw_conv_fwd":
                return fn
            return lambda *a: (seen.append((a[0].value, int(a[12]), int(a[13]))), fn(*a))[1]

    from dl_attack_on_imagenet_amd import _lib
    saved, _lib._lib = _lib._lib, Spy()
    try:
        y = o.pointwise_conv_affine(view, L.w2d, L.wt2d, L.scale, L.shift, relu=False, stride2=True)
    finally:
        _lib._lib = saved
    assert y.shape == (b, 128, oh, ow) and same(nhwc(y).reshape(-1, 128), want)
    (x_ptr, sub_w, sub_hw), = seen
    if in_place:
        assert (x_ptr, sub_w, sub_hw) == (full.data_ptr(), ow, oh * ow)
    else:
        assert x_ptr != full.data_ptr() and (sub_w, sub_hw) == (0, 0)


# ----------------------------------------------------------------------------------------- (a) pointwise, gradient
GRAD_ROWS = ["main", "twin_only", "main_twin", "main_twin_sub", "main_sub", "fp32", "nchw"]


@pytest.mark.parametrize("K,N", [(64, 256), (256, 64)])
@pytest.mark.parametrize("row", GRAD_ROWS)
@pytest.mark.parametrize("res,pre", [(False, False), (True, True)])
def test_pointwise_gradient_equals_one_c_abi_call_bitwise(K, N, row, res, pre):
    """Each row is ONE adil_pw_conv_bwd call with the matching optional pointers (g2, g3 with sub_w / sub_hw, gres, xin)."""
    o, b, h, w = ops(), 2, 12, 10
    L = Layer("bwd/%s" % row, b, h, w, K, N)
    x = nchw(L.x, b, h, w).requires_grad_(True)
    r = nchw(L.res, b, h, w).requires_grad_(True) if res else None
    outputs = 3 if "sub" in row else (2 if "twin" in row else 1)
    got = o.pointwise_conv_affine(x, L.w2d, L.wt2d, L.scale, L.shift, res=r, relu=True, outputs=outputs,
                                  pre=(L.pscale, L.pshift) if pre else None)
    got = (got,) if outputs == 1 else got
    y = nhwc(got[0].detach()).reshape(-1, N)
    assert not bool((R.bits(y) == -32768).any())                       # the forward emits no -0.0: the mask's precondition
    g, g2, g3 = nchw(L.g, b, h, w), nchw(L.g2, b, h, w), nchw(L.g3, b, h // 2, w // 2)
    kw = dict(g=L.g, g2=None)
    if row == "main":
        outs, grads = (got[0],), (g,)
    elif row == "twin_only":
        outs, grads = (got[1],), (g,)
    elif row == "main_twin":
        outs, grads, kw = got, (g, g2), dict(g=L.g, g2=L.g2)
    elif row == "main_twin_sub":
        outs, grads, kw = got, (g, g2, g3), dict(g=L.g, g2=L.g2, g3=L.g3, sub_w=w // 2, sub_hw=(h // 2) * (w // 2))
    elif row == "main_sub":
        outs, grads, kw = (got[0], got[2]), (g, g3), dict(g=L.g, g2=None, g3=L.g3, sub_w=w // 2, sub_hw=(h // 2) * (w // 2))
    elif row == "nchw":
        gc = g.contiguous()
        assert gc.is_contiguous() and not nhwc(gc).is_contiguous()
        outs, grads = (got[0],), (gc,)
    want = abi().step("pw_bwd", wt=L.wt2d, scale=L.scale, y=y, relu=1, xin=L.x if pre else None,
                      pscale=L.pscale if pre else None, pshift=L.pshift if pre else None, want_gres=res,
                      **(kw if row != "fp32" else dict(g=L.g.float().mul(1.0009765625).to(BF16), g2=None)))
    if row == "fp32":        # an fp32 gradient that is NOT bf16-representable: rounded once, to nearest even, by the function
        g32 = nchw(L.g.float().mul(1.0009765625), b, h, w)
        assert g32.dtype == F32 and not torch.equal(g32, g32.to(BF16).float())
        back = o.PointwiseConvFunction.backward(got[0].grad_fn, g32)
        assert len(back) == 11 and all(v is None for v in back[2:])
        gx, gres = back[0], back[1]
    else:
        back = torch.autograd.grad(outs, (x, r) if res else (x,), grads)
        gx, gres = back[0], (back[1] if res else None)
    assert gx.shape == x.shape and same(nhwc(gx).reshape(-1, K), want["gx"]) and bool(gx.float().abs().sum() > 0)
    if res:
        assert gres.shape == r.shape and same(nhwc(gres).reshape(-1, N), want["gres"])
    else:
        assert gres is None


def test_pointwise_gradient_without_a_gradient_and_sub_alone():
    """No gradient at all: every returned gradient is None.  A stride-2 gradient without a full-resolution one: RuntimeError."""
    o, b, h, w = ops(), 2, 12, 10
    L = Layer("none", b, h, w, 64, 256)
    x = nchw(L.x, b, h, w).requires_grad_(True)
    y, y2, ysub = o.pointwise_conv_affine(x, L.w2d, L.wt2d, L.scale, L.shift, outputs=3)
    back = o.PointwiseConvFunction.backward(y.grad_fn, None, None, None)
    assert len(back) == 11 and all(v is None for v in back)
    with pytest.raises(RuntimeError, match="without a full-resolution"):
        torch.autograd.grad(ysub, x, nchw(L.g3, b, h // 2, w // 2))
    with pytest.raises(RuntimeError, match="without a full-resolution"):
        o.PointwiseConvFunction.backward(y.grad_fn, None, None, nchw(L.g3, b, h // 2, w // 2))


# ------------------------------------------------------------------------------------------------ (a) join, conv3x3
def test_pointwise_join_equals_the_c_abi_bitwise():
    o, b, h, w, W = ops(), 2, 12, 10, 64
    C, M = 4 * W, 2 * 12 * 10
    G = R.Gen("wiring/join", "gaussian")
    d = lambda t: t.to(DEV).contiguous()
    h2raw, x = d(G.act(M, W)), d(G.act(M, C))
    w3, w1 = d(G.weight(C, W)), d(G.weight(W, C))
    s2, b2, s3, b3, s1, b1 = d(G.scale(W)), d(G.shift(W)), d(G.scale(C)), d(G.shift(C)), d(G.scale(W)), d(G.shift(W))
    g_out, g_h1 = d(G.act(M, C)), d(G.act(M, W))
    be = abi()
    wf = be.step("join_fwd", h2raw=h2raw, pscale2=s2, pshift2=b2, w3=w3, scale3=s3, shift3=b3, res=x, w1=w1, scale1=s1, shift1=b1)
    wt3, wt1 = w3.t().contiguous(), w1.t().contiguous()
    hx, xx = nchw(h2raw, b, h, w).requires_grad_(True), nchw(x, b, h, w).requires_grad_(True)
    out, h1 = o.pointwise_join(hx, xx, w3, wt3, (s2, b2), s3, b3, w1, wt1, s1, b1)
    assert out.shape == (b, C, h, w) and h1.shape == (b, W, h, w)
    assert same(nhwc(out).reshape(M, C), wf["out"]) and same(nhwc(h1).reshape(M, W), wf["h1"])
    for t in (wf["out"], wf["h1"]):
        assert not bool((R.bits(t) == -32768).any())
    wb = be.step("join_bwd", g_h1=g_h1, h1=wf["h1"], scale1=s1, wt1=wt1, g_out=g_out, out=wf["out"], scale3=s3, wt3=wt3,
                 h2raw=h2raw, pscale2=s2, pshift2=b2)
    gh, gx = torch.autograd.grad((out, h1), (hx, xx), (nchw(g_out, b, h, w), nchw(g_h1, b, h, w)))
    assert gh.shape == hx.shape and gx.shape == xx.shape
    assert same(nhwc(gh).reshape(M, W), wb["gx"]) and same(nhwc(gx).reshape(M, C), wb["gres"])


@pytest.mark.parametrize("C,N", [(64, 128), (128, 64)])
def test_conv3x3_equals_the_c_abi_bitwise(C, N):
    """ops.conv3x3 with the packings of ops.pack_conv3x3_weights against adil_conv3x3 with the packings restated in
    classifier_reference, both directions, C != N."""
    o, b, h, w = ops(), 2, 12, 10
    G = R.Gen("wiring/conv3x3/%d" % C, "gaussian")
    x, g = G.act(b, h, w, C).to(DEV), G.act(b, h, w, N).to(DEV)
    wgt = G.weight(N, C, 3, 3, fan_in=9 * C).to(DEV)
    wp_fwd, wp_bwd = o.pack_conv3x3_weights(wgt)
    assert same(wp_fwd.reshape(N, 9, C), R.pack_taps(wgt)) and same(wp_bwd.reshape(C, 9, N), R.pack_taps_flipped(wgt))
    be = abi()
    xi = x.permute(0, 3, 1, 2).requires_grad_(True)
    y = o.conv3x3(xi, wp_fwd, wp_bwd)
    assert y.shape == (b, N, h, w) and same(nhwc(y), be.step("conv3x3", x=x, w=wgt)["y"])
    (gx,) = torch.autograd.grad(y, xi, g.permute(0, 3, 1, 2))
    assert gx.shape == xi.shape and same(nhwc(gx), be.step("conv3x3_bwd", g=g, w=wgt)["gx"])


# --------------------------------------------------------------------------------------------------- (a) affine_act
@pytest.mark.parametrize("case", ["channels_last", "nchw", "res_other_layout", "res_other_dtype", "no_relu", "no_relu_res"])
def test_affine_act_equals_the_c_abi_bitwise(case):
    o, b, c, h, w = ops(), 2, 64, 6, 5
    n = b * c * h * w
    G = R.Gen("wiring/act/" + case, "gaussian")
    scale, shift = G.scale(c).to(DEV), G.shift(c).to(DEV)
    relu = not case.startswith("no_relu")
    with_res = case != "no_relu"
    flat_x, flat_r, flat_g = (G.act(n).to(DEV) for _ in range(3))
    if case == "nchw":                       # contiguous NCHW storage: inner = H * W
        x, r, g, inner = flat_x.view(b, c, h, w), flat_r.view(b, c, h, w), flat_g.view(b, c, h, w), h * w
        stored = lambda t: t.contiguous().flatten()
    else:                                    # channels_last storage: inner = 1
        x, r, g, inner = nchw(flat_x, b, h, w), nchw(flat_r, b, h, w), nchw(flat_g, b, h, w), 1
        stored = lambda t: nhwc(t).contiguous().flatten()
    r_given = r
    if case == "res_other_layout":
        r_given = r.contiguous()
        assert not r_given.is_contiguous(memory_format=torch.channels_last)
    if case == "res_other_dtype":            # converted first: the bits of the call on the converted tensor
        r_given = (r.float() * 1.0009765625)
        r = r_given.to(BF16)
    be = abi()
    want = be.step("affine_act_fwd", x=stored(x), scale=scale, shift=shift, res=stored(r) if with_res else None, C=c, inner=inner,
                   relu=int(relu), dtype=BF16)["y"]
    xi = x.detach().requires_grad_(True)
    ri = r_given.detach().requires_grad_(True) if with_res else None
    y = o.affine_act(xi, scale, shift, res=ri, relu=relu)
    assert y.shape == x.shape and y.stride() == x.stride() and same(stored(y.detach()), want)
    wb = be.step("affine_act_bwd", g=stored(g), y=want if relu else None, scale=scale, C=c, inner=inner, relu=int(relu),
                 dtype=BF16, want_gres=with_res)
    back = torch.autograd.grad(y, (xi, ri) if with_res else (xi,), g)
    assert back[0].shape == x.shape and same(stored(back[0]), wb["gx"])
    if with_res:
        assert back[1].shape == x.shape and back[1].dtype == r_given.dtype
        if case == "res_other_dtype":        # autograd casts the residual's gradient back to the residual's dtype
            assert torch.equal(stored(back[1]), wb["gres"].float())
        else:
            assert same(stored(back[1]), wb["gres"])


# ------------------------------------------------------------------------------------------------- (a) empty batches
def test_empty_batches_pass_through():
    o, h, w = ops(), 12, 10
    L = Layer("empty", 1, h, w, 64, 128)
    e = lambda c, hh=h, ww=w: torch.empty(0, hh, ww, c, dtype=BF16, device=DEV).permute(0, 3, 1, 2).requires_grad_(True)
    x, r = e(64), e(128)
    ys = o.pointwise_conv_affine(x, L.w2d, L.wt2d, L.scale, L.shift, res=r, outputs=3, pre=(L.pscale, L.pshift))
    assert [tuple(t.shape) for t in ys] == [(0, 128, h, w), (0, 128, h, w), (0, 128, h // 2, w // 2)]
    gx, gr = torch.autograd.grad(ys, (x, r), [torch.empty_like(t) for t in ys])
    assert gx.shape == x.shape and gr.shape == r.shape
    y = o.pointwise_conv_affine(e(64)[:, :, ::2, ::2], L.w2d, L.wt2d, L.scale, L.shift, relu=False, stride2=True)
    assert tuple(y.shape) == (0, 128, h // 2, w // 2)
    W, C = 64, 256
    w3, w1 = torch.zeros(C, W, dtype=BF16, device=DEV), torch.zeros(W, C, dtype=BF16, device=DEV)
    f = lambda n: torch.ones(n, device=DEV)
    hx, xx = e(W), e(C)
    out, h1 = o.pointwise_join(hx, xx, w3, w3.t().contiguous(), (f(W), f(W)), f(C), f(C), w1, w1.t().contiguous(), f(W), f(W))
    assert tuple(out.shape) == (0, C, h, w) and tuple(h1.shape) == (0, W, h, w)
    gh, gx = torch.autograd.grad((out, h1), (hx, xx), (torch.empty_like(out), torch.empty_like(h1)))
    assert gh.shape == hx.shape and gx.shape == xx.shape
    wp_fwd, wp_bwd = o.pack_conv3x3_weights(torch.zeros(128, 64, 3, 3, device=DEV))
    xc = e(64)
    yc = o.conv3x3(xc, wp_fwd, wp_bwd)
    assert tuple(yc.shape) == (0, 128, h, w)
    assert torch.autograd.grad(yc, xc, torch.empty_like(yc))[0].shape == xc.shape
    xa, ra = e(128), e(128)
    ya = o.affine_act(xa, L.scale, L.shift, res=ra)
    assert tuple(ya.shape) == (0, 128, h, w)
    ga, gra = torch.autograd.grad(ya, (xa, ra), torch.empty_like(ya))
    assert ga.shape == xa.shape and gra.shape == ra.shape


# --------------------------------------------------------------------------------------- (a) _ConvAffine.forward
def _bn(n, gen):
    bn = torch.nn.BatchNorm2d(n).eval()
    with torch.no_grad():
        bn.weight.copy_((0.5 + torch.rand(n, generator=gen)) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1))
        bn.bias.copy_(0.2 * torch.randn(n, generator=gen))
        bn.running_mean.copy_(0.2 * torch.randn(n, generator=gen))
        bn.running_var.copy_(0.6 + 0.8 * torch.rand(n, generator=gen))
    return bn


def test_conv_affine_refusals_and_the_unfused_path():
    """pre= / strided_view=True on a layer the fused kernels do not cover: RuntimeError.  A layer whose reshaped weight is
    not contiguous takes the unfused path and equals affine_act(conv(x)) bit for bit."""
    from dl_attack_on_imagenet_amd import zoo
    o = ops()
    gen = torch.Generator().manual_seed(9)
    x = nchw(torch.randn(2 * 12 * 10, 64, generator=gen).to(BF16).to(DEV), 2, 12, 10)
    tables = (torch.ones(64, device=DEV), torch.zeros(64, device=DEV))
    three = zoo._ConvAffine(torch.nn.Conv2d(64, 64, 3, 1, 1, bias=False), _bn(64, gen), True).to(DEV).to(BF16)
    narrow = zoo._ConvAffine(torch.nn.Conv2d(64, 32, 1, bias=False), _bn(32, gen), True).to(DEV).to(BF16)
    strided3 = zoo._ConvAffine(torch.nn.Conv2d(64, 64, 3, 2, 1, bias=False), _bn(64, gen), True).to(DEV).to(BF16)
    for layer in (three, narrow, strided3):
        assert not layer.fused_pointwise(x) and not layer.fused_pointwise_s2(x)
        with pytest.raises(RuntimeError, match="need the fused pointwise kernels"):
            layer(x, pre=tables)
        with pytest.raises(RuntimeError, match="need the fused pointwise kernels"):
            layer(x[:, :, ::2, ::2], strided_view=True)
    conv = torch.nn.Conv2d(64, 128, 1, bias=False)
    base = (torch.randn(64, 128, generator=gen) * 0.125).to(BF16)
    conv.weight = torch.nn.Parameter(base.float().t()[:, :, None, None], requires_grad=False)
    layer = zoo._ConvAffine(conv, _bn(128, gen), True).to(DEV).to(BF16)
    # (128, 64, 1, 1) with strides (1, 128, ..): set on the device, so that no cast or move decides the strides
    layer.conv.weight = torch.nn.Parameter(base.to(DEV).t()[:, :, None, None], requires_grad=False)
    w2d = layer.conv.weight.reshape(128, 64)
    assert layer.fused_pointwise(x) and not w2d.is_contiguous() and torch.equal(layer.wt2d, w2d.t())
    assert layer.scale.dtype == F32
    res = nchw(torch.randn(2 * 12 * 10, 128, generator=gen).to(BF16).to(DEV), 2, 12, 10)
    got = layer(x, res=res, outputs=3)
    want = o.affine_act(layer._conv(x), layer.scale.float(), layer.shift.float(), res=res, relu=True)
    assert len(got) == 3 and same(got[0], want) and got[1] is got[0] and torch.equal(got[2], want[:, :, ::2, ::2])
    with pytest.raises(RuntimeError, match="need the fused pointwise kernels"):
        layer(x, pre=(torch.ones(64, device=DEV), torch.zeros(64, device=DEV)))


# ------------------------------------------------------------------------------------- (b) the product and the tape
class Run:
    pass


def product_run(kind, chain_joins, monkeypatch):
    """FusedResNet(own_strided_conv=True) on p with the stem bypassed and Conv2d.forward patched to raise: block outputs
    (hooks), gradient with respect to p, and what the hooks saw."""
    from dl_attack_on_imagenet_amd import zoo
    net = T.make_net(kind)
    model = zoo.FusedResNet(net, normalize=None, own_strided_conv=True, chain_joins=chain_joins)
    model = model.eval().to(device=DEV, dtype=BF16).to(memory_format=torch.channels_last)
    model.stem, model.maxpool = torch.nn.Identity(), torch.nn.Identity()
    p, g = (t.to(DEV) for t in T.make_inputs(kind))
    r = Run()
    r.net, r.model, r.p, r.g = net, model, p, g
    r.returned, r.down_calls = [], []
    hooks = []
    for blk in model.layers:
        hooks.append(blk.register_forward_hook(lambda m, a, out: r.returned.append(out)))
        if blk.down is not None:
            hooks.append(blk.down.register_forward_pre_hook(
                lambda m, a, kw: r.down_calls.append((m, tuple(a[0].shape), tuple(a[0].stride()), bool(kw.get("strided_view")))),
                with_kwargs=True))

    def refuse(self, *a, **k):
        raise AssertionError("library convolution called: %r" % (self,))

    x = p.permute(0, 3, 1, 2).requires_grad_(True)
    assert x.is_contiguous(memory_format=torch.channels_last)
    with monkeypatch.context() as mp:
        mp.setattr(torch.nn.Conv2d, "forward", refuse)
        model(x)
        first = [o[0] if isinstance(o, tuple) else o for o in r.returned]
        (gp,) = torch.autograd.grad(first[-1], x, g.permute(0, 3, 1, 2))
    for hk in hooks:
        hk.remove()
    torch.cuda.synchronize()
    r.outs = [nhwc(t.detach()) for t in first]
    r.grad = nhwc(gp)
    return r


def tape_run(kind, joins, keep_log=False):
    from dl_attack_on_imagenet_amd import zoo
    be = abi(keep_log=keep_log)
    tables = T.layer_tables(T.make_net(kind), zoo._bn_affine, device=DEV, wdtype=BF16)
    p, g = (t.to(DEV) for t in T.make_inputs(kind))
    tape = T.run_tape(be, tables, p, g, joins=joins)
    torch.cuda.synchronize()
    return tape, be


_TAPES = {}


def shared_tape(kind, joins):
    """The abi tape of a network, computed once and left unchanged."""
    if (kind, joins) not in _TAPES:
        _TAPES[kind, joins] = tape_run(kind, joins)[0]
    return _TAPES[kind, joins]


def first_mismatch(r, tape):
    """None, or the name of the first tensor of the product that differs from the tape's (values: +0 equals -0)."""
    for i, (a, b) in enumerate(zip(r.outs, tape.outs)):
        if a.shape != b.shape or not torch.equal(a, b):
            return "output of block %d" % i
    if r.grad.shape != tape.grad.shape or not torch.equal(r.grad, tape.grad):
        return "gradient with respect to p"
    return None


@pytest.mark.parametrize("kind,chain_joins", [("bottleneck", True), ("bottleneck", False), ("basic", True)])
def test_fused_resnet_equals_the_tape_bitwise(kind, chain_joins, monkeypatch):
    from dl_attack_on_imagenet_amd import zoo
    t0 = time.time()
    r = product_run(kind, chain_joins, monkeypatch)
    tape = shared_tape(kind, chain_joins)
    blocks = list(r.model.layers)
    assert len(r.outs) == len(tape.outs) == len(blocks)
    # the premises: what the run was meant to exercise did run
    joined = [isinstance(o, zoo._Joined) for o in r.returned]
    triples = [isinstance(o, tuple) and not isinstance(o, zoo._Joined) and len(o) == 3 for o in r.returned]
    if kind == "bottleneck":
        assert joined == ([True, True] + [False] * 6 if chain_joins else [False] * 8), joined
        assert [b.emit_sub for b in blocks] == [False, False, True, False, True, False, True, False]
        assert triples == [b.emit_sub for b in blocks], triples
        assert isinstance(r.returned[-1], tuple) and len(r.returned[-1]) == 2
        assert blocks[0].c3.conv.in_channels == 64 and r.model.chain_joins == chain_joins
    else:
        assert not any(joined) and not any(triples) and all(isinstance(o, torch.Tensor) for o in r.returned)
    strided = [c for c in r.down_calls if c[0].pointwise_s2]
    assert len(strided) == 3 and len(r.down_calls) == (4 if kind == "bottleneck" else 3)
    for m, shape, stride, flag in strided:                             # the gather: a [:, :, ::2, ::2] view, read in place (sub_w > 0)
        b, c, oh, ow = shape
        assert flag and stride == (4 * oh * ow * c, 1, 4 * ow * c, 2 * c), (shape, stride, flag)
    for t in r.outs:
        assert not bool((R.bits(t) == -32768).any()), "a block output holds -0.0"
    assert bool(torch.isfinite(r.grad.float()).all()) and bool(r.grad.float().abs().sum() > 0)
    bad = first_mismatch(r, tape)
    assert bad is None, f"{kind} chain_joins={chain_joins}: FusedResNet and the C-ABI tape differ first at the {bad}"
    torch.cuda.synchronize()
    print(f"{kind} chain_joins={chain_joins}: {len(blocks)} block outputs and the gradient equal the tape's; {time.time() - t0:.2f} s")


def test_tape_with_and_without_joins_is_the_same_bits():
    """adil_pw_join_* are bitwise the two pointwise calls they replace, at the composite shapes too."""
    a, b = shared_tape("bottleneck", True), shared_tape("bottleneck", False)
    for t, u in zip(a.outs + [a.grad], b.outs + [b.grad]):
        assert same(t, u)


# --------------------------------------------------------------------------- (c) the tape's steps are the restatements
@pytest.mark.parametrize("kind", ["bottleneck", "basic"])
def test_every_tape_step_is_within_the_bound_of_its_restatement(kind):
    tape, be = tape_run(kind, True, keep_log=True)
    worst, count, ar = {}, {}, R.Arith()
    for name, kw, outs in be.log:
        ref = T.OPS[name](ar, **kw)
        for k, got in outs.items():
            q = R.gaussian_ratio(got, ref[k])
            worst[name] = max(worst.get(name, 0.0), q)
        count[name] = count.get(name, 0) + 1
    for name in sorted(worst):
        print(f"{kind}: {name:15s} {count[name]:3d} steps, worst max err / bound = {worst[name]:.3f}")
    assert set(worst) == ({"pw_fwd", "pw_bwd", "join_fwd", "join_bwd", "conv3x3", "conv3x3_bwd", "s2_fwd", "s2_bwd"}
                          if kind == "bottleneck" else
                          {"pw_fwd", "pw_bwd", "conv3x3", "conv3x3_bwd", "s2_fwd", "s2_bwd", "affine_act_fwd", "affine_act_bwd"})
    for name, q in worst.items():
        assert q <= 1.0, f"{kind}: a {name} step is {q:.3f} times its bound away from the restatement"


# ------------------------------------------------------------------------------------------ (d) the comparison notices
def _without(which):
    o = ops()
    real = o.PointwiseConvFunction.backward

    def backward(ctx, g, g_twin=None, g_sub=None):
        return real(ctx, g, None if which == "g_twin" else g_twin, None if which == "g_sub" else g_sub)
    return staticmethod(backward)


@pytest.mark.parametrize("which", ["g_sub", "g_twin"])
def test_a_dropped_optional_gradient_is_reported(which, monkeypatch):
    """PointwiseConvFunction.backward wrapped so that it discards g_sub / g_twin (it only omits an optional pointer of a
    call that is otherwise the correct one): the comparison of (b) must name a mismatch, and it is the gradient."""
    monkeypatch.setattr(ops().PointwiseConvFunction, "backward", _without(which))
    r = product_run("bottleneck", True, monkeypatch)
    bad = first_mismatch(r, shared_tape("bottleneck", True))
    print(f"mutant without {which}: first mismatch at the {bad}")
    assert bad == "gradient with respect to p", bad


def test_what_the_loose_recipe_makes_of_the_two_mutants(monkeypatch):
    """For the record (printed, not asserted): cosine and norm ratio, against the fp32 network, of the recipe of
    test_fused_resnet50_gradient_matches_fp32 (ResNet-50, its own 4 x 3 x 64 x 64 input) for the sound product and for the two
    mutants above.  That test requires cos >= (plain bf16 network's cos) - 0.02 and a norm within 5 % + twice the plain
    network's miss; measured on the MI355X (profiles/resnet_wiring.md): sound 0.954 / 0.98, without g_sub 0.31 / 0.27,
    without g_twin 0.04 / 0.04 -- it does notice these two."""
    from dl_attack_on_imagenet_amd import zoo
    ref = zoo.build_classifier("resnet50", num_classes=10, seed=5, device=DEV, dtype=torch.float32)
    m1 = zoo.build_classifier("resnet50", num_classes=10, seed=5, device=DEV, dtype=torch.bfloat16, channels_last=True,
                              fuse_bn_act=True, fuse_stem=True)
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(0)).to(DEV).bfloat16()

    def gradient(m, xi):
        xi = xi.requires_grad_(True)
        return torch.autograd.grad(m(xi).float().square().sum(), xi)[0].float()

    gr = gradient(ref, x.float())
    for which in (None, "g_sub", "g_twin"):
        with monkeypatch.context() as mp:
            if which:
                mp.setattr(ops().PointwiseConvFunction, "backward", _without(which))
            g1 = gradient(m1, x.clone())
        c1 = float(F.cosine_similarity(g1.flatten(), gr.flatten(), dim=0))
        print(f"loose recipe, {'sound product' if which is None else 'without ' + which}: cos {c1:.5f}, "
              f"|g| / |g fp32| {float(g1.norm()) / float(gr.norm()):.4f}")
        assert bool(torch.isfinite(g1).all())
