"""GPU: the stride-2 3x3 convolution kernels (adil_conv3x3_s2_fwd / adil_conv3x3_s2_bwd, csrc/adil_convs.hip) against
torch's fp32 convolution on the same bf16-rounded operands, and the FusedResNet that runs on them
(`own_strided_conv=True`): no library convolution left, the switch-off network untouched, results bitwise equal across
processes."""
import contextlib
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def ops():
    from dl_attack_on_imagenet_amd import ops as o
    return o


def _lib():
    return __import__("dl_attack_on_imagenet_amd._lib", fromlist=["x"]).load()


@contextlib.contextmanager
def _deterministic_library():
    """The library convolutions alone are not repeatable call to call: on ResNet-50 at 64 x 64 the stride-2 3x3 layer of
    stage 3 (block 7) gave different bits for the SAME network and input within one process (first differing block
    output: 7, in 2 of 2 repeats), and identical bits under torch.backends.cudnn.deterministic.  Bitwise comparisons of
    two library-path networks therefore pin the library to its deterministic solvers; the own kernels need no such flag."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = prev


def _bf16_depth_bound(layers: int) -> float:
    """The bound of tests/test_gpu_stem.py, restated: mean |logit error| of a bf16-activation network against its fp32
    twin relative to the rms logit; `layers` roundings of relative size 2^-9 in series add in quadrature, times 2 for a
    relative gain above 1 in a random-weight network."""
    return 2.0 * 2.0 ** -9 * layers ** 0.5


SHAPES = [(2, 56, 56, 128, 128), (2, 28, 28, 256, 256), (2, 14, 14, 512, 512), (1, 56, 56, 64, 128), (3, 6, 10, 64, 128),
          (1, 2, 2, 64, 64), (2, 4, 2, 192, 64), (5, 8, 8, 128, 256), (3, 22, 18, 128, 64)]


@pytest.mark.parametrize("b,h,w_,c,n", SHAPES)
def test_conv3x3_s2_forward_and_input_gradient(b, h, w_, c, n):
    """Through the C ABI against torch's fp32 F.conv2d(stride=2, padding=1) and its autograd on the same bf16-rounded
    operands (x, g ~ N(0,1), w ~ N(0,1)/sqrt(9C)); bound |err| <= 2^-7 |ref| + 2e-3 elementwise (the correctly rounded
    result uses at most 0.44 of it on these shapes).  Pixel counts that are no multiple of the 128-row tile, image
    borders and image-to-image boundaries inside a tile occur ((3,6,10): 45 rows of 3 images in one tile; (3,22,18): 297
    rows).  Rows past the end of y / gx keep their canary; a second call gives identical bits."""
    o, lib = ops(), _lib()
    oh, ow = h // 2, w_ // 2
    gen = torch.Generator().manual_seed(b * h * w_ + c + n)
    x = torch.randn(b, h, w_, c, generator=gen).bfloat16().to(DEV)
    wt = (torch.randn(n, c, 3, 3, generator=gen) / (9 * c) ** 0.5).bfloat16().float().to(DEV)
    wf, wb = o.pack_conv3x3_s2_weights(wt)
    assert wf.shape == (n, 9 * c) and wb.shape == (c, 9 * n) and wf.dtype == wb.dtype == torch.bfloat16
    m = b * oh * ow
    y = torch.full((m + 5, n), 7.0, dtype=torch.bfloat16, device=DEV)
    assert lib.adil_conv3x3_s2_fwd(o._ptr(x), o._ptr(wf), o._ptr(y), b, h, w_, c, n, o._stream()) == 0
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), wt, stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, n)
    assert ref.shape[0] == m
    err = (y[:m].float() - ref).abs()
    tol = 2 ** -7 * ref.abs() + 2e-3
    print("fwd", (b, h, w_, c, n), "max err %.3e, max err/tol %.3f" % (float(err.max()), float((err / tol).max())))
    assert bool((err <= tol).all()), float(err.max())
    assert bool((y[m:] == 7.0).all())
    y2 = torch.full_like(y, 7.0)
    assert lib.adil_conv3x3_s2_fwd(o._ptr(x), o._ptr(wf), o._ptr(y2), b, h, w_, c, n, o._stream()) == 0
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16))

    g = torch.randn(b, oh, ow, n, generator=gen).bfloat16().to(DEV)
    m4 = b * h * w_
    gx = torch.full((m4 + 5, c), 7.0, dtype=torch.bfloat16, device=DEV)
    assert lib.adil_conv3x3_s2_bwd(o._ptr(g), o._ptr(wb), o._ptr(gx), b, h, w_, c, n, o._stream()) == 0
    xin = torch.zeros(b, c, h, w_, device=DEV, requires_grad=True)
    F.conv2d(xin, wt, stride=2, padding=1).backward(g.float().permute(0, 3, 1, 2))
    gref = xin.grad.permute(0, 2, 3, 1).reshape(-1, c)
    gerr = (gx[:m4].float() - gref).abs()
    gtol = 2 ** -7 * gref.abs() + 2e-3
    print("bwd", (b, h, w_, c, n), "max err %.3e, max err/tol %.3f" % (float(gerr.max()), float((gerr / gtol).max())))
    assert bool((gerr <= gtol).all()), float(gerr.max())
    assert bool((gx[m4:] == 7.0).all())
    gx2 = torch.full_like(gx, 7.0)
    assert lib.adil_conv3x3_s2_bwd(o._ptr(g), o._ptr(wb), o._ptr(gx2), b, h, w_, c, n, o._stream()) == 0
    assert torch.equal(gx.view(torch.int16), gx2.view(torch.int16))


def test_conv3x3_s2_autograd_function_and_empty_batch():
    """ops.conv3x3_s2 on channels_last tensors: shapes, the gradient through autograd, an empty batch."""
    o = ops()
    gen = torch.Generator().manual_seed(1)
    wt = (torch.randn(128, 64, 3, 3, generator=gen) / 24.0).bfloat16().float().to(DEV)
    wf, wb = o.pack_conv3x3_s2_weights(wt)
    x = torch.randn(3, 64, 12, 8, generator=gen).bfloat16().to(DEV).contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    y = o.conv3x3_s2(x, wf, wb)
    assert y.shape == (3, 128, 6, 4) and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    xr = x.detach().float().requires_grad_(True)
    yr = F.conv2d(xr, wt, stride=2, padding=1)
    assert bool(((y.float() - yr).abs() <= 2 ** -7 * yr.abs() + 2e-3).all())
    g = torch.randn(yr.shape, generator=gen).bfloat16().to(DEV)
    (gx,) = torch.autograd.grad(y, x, g)
    (gr,) = torch.autograd.grad(yr, xr, g.float())
    assert gx.shape == x.shape and gx.dtype == torch.bfloat16
    assert bool(((gx.float() - gr).abs() <= 2 ** -7 * gr.abs() + 2e-3).all())
    e = torch.zeros(0, 64, 12, 8, dtype=torch.bfloat16, device=DEV, requires_grad=True)
    ye = o.conv3x3_s2(e, wf, wb)
    assert ye.shape == (0, 128, 6, 4)
    (ge,) = torch.autograd.grad(ye.sum(), e)
    assert ge.shape == e.shape


def test_conv3x3_s2_refuses_what_it_does_not_cover():
    """Odd H or W, C % 64 != 0, N % 64 != 0, a width past ADIL_CONV3X3_S2_MAX_W: ADIL_EINVAL from both entry points and
    the outputs untouched; `_ConvAffine` / the network then keep the library with the switch on, bitwise the
    switch-off result."""
    from dl_attack_on_imagenet_amd import zoo
    o, lib = ops(), _lib()
    assert o.CONV3X3_S2_MAX_W == 63
    big = torch.zeros(2 * 64 * 66 * 128, dtype=torch.bfloat16, device=DEV)        # covers every operand below
    for (b, h, w_, c, n) in [(2, 7, 8, 64, 64), (2, 8, 7, 64, 64), (1, 8, 8, 96, 64), (1, 8, 8, 64, 96), (1, 8, 64, 64, 64),
                             (1, 8, 66, 64, 64), (0, 8, 8, 64, 64), (1, 8, 8, 0, 64)]:
        y = torch.full((4096,), 7.0, dtype=torch.bfloat16, device=DEV)
        assert lib.adil_conv3x3_s2_fwd(o._ptr(big), o._ptr(big), o._ptr(y), b, h, w_, c, n, o._stream()) == EINVAL
        assert lib.adil_conv3x3_s2_bwd(o._ptr(big), o._ptr(big), o._ptr(y), b, h, w_, c, n, o._stream()) == EINVAL
        torch.cuda.synchronize()
        assert bool((y == 7.0).all())
    y = torch.full((4096,), 7.0, dtype=torch.bfloat16, device=DEV)
    assert lib.adil_conv3x3_s2_fwd(None, o._ptr(big), o._ptr(y), 1, 8, 8, 64, 64, o._stream()) == EINVAL
    assert lib.adil_conv3x3_s2_bwd(o._ptr(big), None, o._ptr(y), 1, 8, 8, 64, 64, o._stream()) == EINVAL

    # the layer wrapper: switch on, uncovered inputs -> self.conv(x), bitwise
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(64, 128, 3, stride=2, padding=1, bias=False)
    bn = torch.nn.BatchNorm2d(128).eval()
    layer = zoo._ConvAffine(conv, bn, True).to(DEV).to(torch.bfloat16).to(memory_format=torch.channels_last)
    assert layer.dense3x3_s2 and not layer.own_strided_conv
    layer.use_own_strided_conv_()
    assert layer.own_strided_conv
    for shape in [(2, 64, 9, 8), (2, 64, 8, 9), (1, 64, 8, 64)]:
        x = torch.randn(shape, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
        assert torch.equal(layer.raw_conv(x), layer.conv(x))
    x = torch.randn(2, 64, 8, 8, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    own = layer.raw_conv(x)                                            # covered: the kernel (same bound as above)
    ref = F.conv2d(x.float(), layer.conv.weight.float(), stride=2, padding=1)
    assert own.shape == ref.shape and bool(((own.float() - ref).abs() <= 2 ** -7 * ref.abs() + 2e-3).all())

    # the network: 36 x 36 images give the stride-2 layers 9 x 9, 5 x 5 and 3 x 3 inputs
    kw = dict(num_classes=10, seed=3, device=DEV, dtype=torch.bfloat16, channels_last=True, fuse_bn_act=True, fuse_stem=True)
    off = zoo.build_classifier("resnet18", **kw)
    on = zoo.build_classifier("resnet18", own_strided_conv=True, **kw)
    xi = torch.rand(4, 3, 36, 36, generator=torch.Generator().manual_seed(0)).to(DEV).bfloat16()
    x0, x1 = xi.clone().requires_grad_(True), xi.clone().requires_grad_(True)
    with _deterministic_library():
        l0, l1 = off(x0), on(x1)
        assert torch.equal(l0, l1)
        (g0,) = torch.autograd.grad(l0.float().square().sum(), x0)
        (g1,) = torch.autograd.grad(l1.float().square().sum(), x1)
        assert torch.equal(g0, g1)


@pytest.mark.parametrize("name,depth", [("resnet50", 53), ("resnet18", 20)])
def test_fused_resnets_without_library_convolutions(name, depth, monkeypatch):
    """fuse_bn_act + fuse_stem + own_strided_conv: forward and the input gradient run with torch.nn.Conv2d.forward patched
    to raise; logits within the bf16 depth bound of the fp32 network, gradient direction as good as the switch-off
    network's.  With the switch off the same patch raises: the stride-2 layers are the only library convolutions."""
    from dl_attack_on_imagenet_amd import zoo
    ref = zoo.build_classifier(name, num_classes=10, seed=5, device=DEV, dtype=torch.float32)
    kw = dict(num_classes=10, seed=5, device=DEV, dtype=torch.bfloat16, channels_last=True, fuse_bn_act=True, fuse_stem=True)
    off = zoo.build_classifier(name, **kw)
    on = zoo.build_classifier(name, own_strided_conv=True, **kw)
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(0)).to(DEV).bfloat16()
    xr, x0, x1 = (x.float().requires_grad_(True), x.clone().requires_grad_(True), x.clone().requires_grad_(True))
    lr = ref(xr)
    (gr,) = torch.autograd.grad(lr.square().sum(), xr)
    l0 = off(x0).float()
    (g0,) = torch.autograd.grad(l0.square().sum(), x0)

    def refuse(self, *a, **k):
        raise AssertionError("library convolution called: %r" % (self,))

    monkeypatch.setattr(torch.nn.Conv2d, "forward", refuse)
    l1 = on(x1).float()
    (g1,) = torch.autograd.grad(l1.square().sum(), x1)
    with pytest.raises(AssertionError, match="library convolution called"):
        off(x.clone())
    monkeypatch.undo()
    e0, e1 = float((l0 - lr).abs().mean().detach()), float((l1 - lr).abs().mean().detach())
    rms = float(lr.square().mean().sqrt().detach())
    cos = lambda a, b: float(F.cosine_similarity(a.float().flatten(), b.float().flatten(), dim=0))
    c0, c1 = cos(g0, gr), cos(g1, gr)
    print("%s logit error vs fp32: switch off %.4f on %.4f, rms %.4f, bound %.4f; gradient cosine off %.5f on %.5f"
          % (name, e0, e1, rms, _bf16_depth_bound(depth) * rms, c0, c1))
    assert e1 <= _bf16_depth_bound(depth) * rms, (e0, e1, rms)
    assert g1.shape == x.shape and g1.dtype == x.dtype
    assert abs(c1 - c0) <= 0.02, (c0, c1)


def test_switch_off_is_bitwise_the_parent_path():
    """own_strided_conv=False and a network built without the argument: identical logits and input gradient, bit for
    bit (with the library pinned to repeatable solvers, see _deterministic_library: without that the parent path does not
    even equal itself on ResNet-50)."""
    from dl_attack_on_imagenet_amd import zoo
    kw = dict(num_classes=10, seed=5, device=DEV, dtype=torch.bfloat16, channels_last=True, fuse_bn_act=True, fuse_stem=True)
    for name in ("resnet50", "resnet18"):
        a = zoo.build_classifier(name, **kw)
        b = zoo.build_classifier(name, own_strided_conv=False, **kw)
        assert sorted(a.state_dict()) == sorted(b.state_dict())
        x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(0)).to(DEV).bfloat16()
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        with _deterministic_library():
            la, lb = a(xa), b(xb)
            assert torch.equal(la, lb)
            (ga,) = torch.autograd.grad(la.float().square().sum(), xa)
            (gb,) = torch.autograd.grad(lb.float().square().sum(), xb)
            assert torch.equal(ga, gb)


def test_own_classifier_is_bitwise_across_processes():
    """Two fresh child processes, one after the other (the second only if the first exited 0), each under `timeout`:
    the all-own ResNet-50 from a seed, forward + input gradient of a seeded batch of 32 images at 224 x 224, one hash per
    block output plus logits and input gradient — all equal between the two (the head's F.linear is the one library
    call left; the first differing line would name the layer)."""
    child = os.path.join(ROOT, "tests", "own_classifier_child.py")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    outs = []
    for _ in range(2):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, child], env=env, capture_output=True, text=True,
                           timeout=330, cwd=ROOT)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("hash ")]
        assert len(lines) == 16 + 2, r.stdout[-2000:]          # 16 blocks, logits, input gradient
        outs.append(lines)
    for a, b in zip(*outs):
        assert a == b, (a, b)
