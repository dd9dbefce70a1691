"""GPU: the depthwise 3x3 kernels (adil_dw3x3_fwd / adil_dw3x3_bwd, csrc/adil_depthwise.hip) through the C ABI against
the fp64 restatement of tests/depthwise_reference.py — bit for bit on the exact legs, under the derived elementwise bound
on the gaussian leg — and the MobileNetV2 that runs its 17 depthwise layers on them (`own_depthwise=True`)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import depthwise_reference as dref
from classifier_reference import BF16, CANARY, Arith

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PAD = 5                          # canary pixels behind every output
EPS_LEARNER = 8 / 255            # the reference CLI's radius (demo_dL_attack.py: eps 8/255, linf)


def ops():
    from dl_attack_on_imagenet_amd import ops as o
    return o


def _lib():
    return __import__("dl_attack_on_imagenet_amd._lib", fromlist=["x"]).load()


def _need(gb):
    free, _ = torch.cuda.mem_get_info()
    if free < gb * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.0f} GB free, the test needs {gb} GB")


def _bf16_depth_bound(layers: int) -> float:
    """The bound of tests/test_gpu_stem.py, restated: mean |logit error| of a bf16-activation network against its fp32
    twin relative to the rms logit; `layers` roundings of relative size 2^-9 in series add in quadrature, times 2 for a
    relative gain above 1 in a random-weight network."""
    return 2.0 * 2.0 ** -9 * layers ** 0.5


# (B, H, W, C, stride, relu6, bias): the distinct depthwise shapes of MobileNetV2 at 224 x 224, odd grids, channel counts
# that are no multiple of 64, both strides, both activations, no bias
ROWS = [(2, h, h, c, s, 1, True) for (c, h, s) in dref.MOBILENET_SHAPES] + [
    (2, 15, 13, 96, 1, 1, True), (2, 15, 13, 96, 2, 1, True), (2, 7, 7, 960, 1, 1, True), (2, 7, 7, 576, 2, 1, True),
    (3, 1, 5, 8, 1, 1, True), (3, 1, 5, 8, 2, 0, True), (3, 5, 1, 24, 1, 0, True), (3, 5, 1, 24, 2, 1, True),
    (2, 14, 14, 8, 1, 0, False), (2, 14, 14, 8, 2, 1, False), (5, 9, 11, 24, 1, 1, False), (5, 9, 11, 24, 2, 0, True),
    (2, 28, 28, 144, 1, 0, False), (2, 28, 27, 144, 2, 1, True), (1, 1, 1, 8, 1, 1, True), (1, 1, 1, 8, 2, 1, True),
    (1, 2, 3, 16, 2, 1, True), (4, 14, 14, 96, 1, 1, True), (1, 113, 113, 32, 2, 1, True)]


def _run_fwd(op, B, H, W, C, s, relu6):
    o, lib = ops(), _lib()
    OH, OW = dref.out_size(H, s), dref.out_size(W, s)
    x, w = op.x.to(DEV), op.w9c.to(DEV)
    bias = None if op.bias is None else op.bias.to(DEV)
    y = torch.full((B * OH * OW + PAD, C), CANARY, dtype=BF16, device=DEV)
    assert lib.adil_dw3x3_fwd(o._ptr(x), o._ptr(w), o._ptr(bias), o._ptr(y), B, H, W, C, s, relu6, o._stream()) == 0
    torch.cuda.synchronize()
    assert bool((y[B * OH * OW:] == CANARY).all()), "forward wrote past the end of y"
    return y[:B * OH * OW].reshape(B, OH, OW, C)


def _run_bwd(op, y, B, H, W, C, s, relu6):
    o, lib = ops(), _lib()
    g, w = op.g.to(DEV), op.w9c.to(DEV)
    yd = None if y is None else y.to(DEV).contiguous()
    gx = torch.full((B * H * W + PAD, C), CANARY, dtype=BF16, device=DEV)
    assert lib.adil_dw3x3_bwd(o._ptr(g), o._ptr(yd), o._ptr(w), o._ptr(gx), B, H, W, C, s, relu6, o._stream()) == 0
    torch.cuda.synchronize()
    assert bool((gx[B * H * W:] == CANARY).all()), "gradient wrote past the end of gx"
    return gx[:B * H * W].reshape(B, H, W, C)


@pytest.mark.parametrize("B,H,W,C,s,relu6,with_bias", ROWS)
def test_dw3x3_against_the_fp64_restatement(B, H, W, C, s, relu6, with_bias):
    """Forward and input gradient of one row on the exact legs (clamp set when the row has a ReLU6, rounding set always,
    with relu6 = 0) and on the gaussian leg.  Every premise is asserted on the reference before the kernel is looked at."""
    row = "dw/%s" % ((B, H, W, C, s, relu6, with_bias),)
    ar = Arith()
    legs = ([("clamp", 1)] if relu6 else []) + [("rounding", 0)]
    for leg, r6 in legs:
        name = row + "/" + leg
        op = dref.operands(name, leg, B, H, W, C, s, with_bias)
        ref = dref.dw_fwd(ar, op.x, op.w9c, op.bias, s, r6)
        worst, inexact = dref.assert_premise(name + "/fwd", ref, leg)
        if leg == "clamp" and ref.pre.numel() >= 4096:
            shares = dref.branch_shares(ref)
            assert min(shares) >= 0.10, (name, shares)
        y = dref.mask_source(name, leg, dref.finish(ar, ref)) if r6 else None
        refb = dref.dw_bwd(ar, op.g, y, op.w9c, H, W, s, r6)
        worstb, inexactb = dref.assert_premise(name + "/bwd", refb, leg)
        print(name, "sum |terms| fwd %.0f bwd %.0f, outputs that need rounding fwd %.2f bwd %.2f" % (worst, worstb, inexact, inexactb))
        dref.compare_exact(name + "/fwd", _run_fwd(op, B, H, W, C, s, r6), ref)
        dref.compare_exact(name + "/bwd", _run_bwd(op, y, B, H, W, C, s, r6), refb)
    name = row + "/gaussian"
    op = dref.operands(name, "gaussian", B, H, W, C, s, with_bias)
    ref = dref.dw_fwd(ar, op.x, op.w9c, op.bias, s, relu6)
    got = _run_fwd(op, B, H, W, C, s, relu6)
    rf = dref.gaussian_ratio(got, ref)
    y = got.cpu() if relu6 else None                     # the mask source: the kernel's own stored output, on both sides
    refb = dref.dw_bwd(ar, op.g, y, op.w9c, H, W, s, relu6)
    rb = dref.gaussian_ratio(_run_bwd(op, y, B, H, W, C, s, relu6), refb)
    print(name, "max |err| / bound: fwd %.3f bwd %.3f" % (rf, rb))
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)


def test_dw3x3_refuses_and_leaves_outputs_untouched():
    """C = 12, stride 3, a NULL mandatory pointer, non-positive sizes: ADIL_EINVAL from both entry points, canaries intact."""
    o, lib = ops(), _lib()
    big = torch.zeros(2 * 16 * 16 * 16, dtype=BF16, device=DEV)
    w = torch.zeros(9 * 16, dtype=torch.float32, device=DEV)
    out = torch.full((2 * 16 * 16 * 16,), CANARY, dtype=BF16, device=DEV)
    P = o._ptr
    for (B, H, W, C, s) in [(2, 8, 8, 12, 1), (2, 8, 8, 8, 3), (2, 8, 8, 8, 0), (0, 8, 8, 8, 1), (2, 0, 8, 8, 1), (2, 8, 0, 8, 2),
                            (2, 8, 8, 0, 1), (2, 8, 8, 4, 2)]:
        for r6 in (0, 1):
            assert lib.adil_dw3x3_fwd(P(big), P(w), P(w), P(out), B, H, W, C, s, r6, o._stream()) == EINVAL
            assert lib.adil_dw3x3_bwd(P(big), P(big), P(w), P(out), B, H, W, C, s, r6, o._stream()) == EINVAL
    assert lib.adil_dw3x3_fwd(None, P(w), P(w), P(out), 2, 8, 8, 8, 1, 1, o._stream()) == EINVAL          # NULL x
    assert lib.adil_dw3x3_fwd(P(big), None, P(w), P(out), 2, 8, 8, 8, 1, 1, o._stream()) == EINVAL
    assert lib.adil_dw3x3_fwd(P(big), P(w), P(w), None, 2, 8, 8, 8, 1, 1, o._stream()) == EINVAL
    assert lib.adil_dw3x3_bwd(None, P(big), P(w), P(out), 2, 8, 8, 8, 1, 1, o._stream()) == EINVAL
    assert lib.adil_dw3x3_bwd(P(big), None, P(w), P(out), 2, 8, 8, 8, 1, 1, o._stream()) == EINVAL        # relu6 needs y
    assert lib.adil_dw3x3_bwd(P(big), P(big), None, P(out), 2, 8, 8, 8, 1, 1, o._stream()) == EINVAL
    assert lib.adil_dw3x3_bwd(P(big), P(big), P(w), None, 2, 8, 8, 8, 1, 1, o._stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    # the accepted forms of the optional pointers: bias NULL, y NULL without a ReLU6
    assert lib.adil_dw3x3_fwd(P(big), P(w), None, P(out), 2, 8, 8, 8, 1, 1, o._stream()) == 0
    assert lib.adil_dw3x3_bwd(P(big), None, P(w), P(out), 2, 8, 8, 8, 1, 0, o._stream()) == 0
    torch.cuda.synchronize()
    assert bool((out[:2 * 8 * 8 * 8] == 0).all()) and bool((out[2 * 8 * 8 * 8:] == CANARY).all())


def test_dw3x3_beyond_2_31_elements():
    """B = 2048 at 112 x 112 x 96, stride 2: x and gx hold 2.47e9 elements (offsets pass 2^31, and 2^32 bytes).  The first
    and the last two images of the big call equal, bit for bit, a call on those two images alone (whose correctness the row
    table establishes), forward and gradient."""
    _need(24)
    o, lib = ops(), _lib()
    B, H, W, C, s = 2048, 112, 112, 96, 2
    OH = OW = 56
    assert B * H * W * C > 2 ** 31
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    x = torch.empty((B, H, W, C), dtype=BF16, device=DEV)
    for b0 in range(0, B, 256):
        x[b0:b0 + 256] = torch.randint(-3, 4, (256, H, W, C), generator=gen, device=DEV, dtype=torch.int8).to(BF16)
    op = dref.operands("big", "clamp", 1, 3, 3, C, 1)
    w, bias = op.w9c.to(DEV), op.bias.to(DEV)
    y = torch.full((B, OH, OW, C), CANARY, dtype=BF16, device=DEV)
    assert lib.adil_dw3x3_fwd(o._ptr(x), o._ptr(w), o._ptr(bias), o._ptr(y), B, H, W, C, s, 1, o._stream()) == 0
    for b0 in (0, B - 2):
        part = torch.full((2, OH, OW, C), CANARY, dtype=BF16, device=DEV)
        xs = x[b0:b0 + 2].contiguous()
        assert lib.adil_dw3x3_fwd(o._ptr(xs), o._ptr(w), o._ptr(bias), o._ptr(part), 2, H, W, C, s, 1, o._stream()) == 0
        assert torch.equal(y[b0:b0 + 2].view(torch.int16), part.view(torch.int16)), b0
    assert not bool((y[B // 2] == CANARY).any())
    g = torch.empty((B, OH, OW, C), dtype=BF16, device=DEV)
    for b0 in range(0, B, 256):
        g[b0:b0 + 256] = torch.randint(-3, 4, (256, OH, OW, C), generator=gen, device=DEV, dtype=torch.int8).to(BF16)
    del x
    gx = torch.full((B, H, W, C), CANARY, dtype=BF16, device=DEV)
    assert lib.adil_dw3x3_bwd(o._ptr(g), o._ptr(y), o._ptr(w), o._ptr(gx), B, H, W, C, s, 1, o._stream()) == 0
    for b0 in (0, B - 2):
        part = torch.full((2, H, W, C), CANARY, dtype=BF16, device=DEV)
        gs, ys = g[b0:b0 + 2].contiguous(), y[b0:b0 + 2].contiguous()
        assert lib.adil_dw3x3_bwd(o._ptr(gs), o._ptr(ys), o._ptr(w), o._ptr(part), 2, H, W, C, s, 1, o._stream()) == 0
        assert torch.equal(gx[b0:b0 + 2].view(torch.int16), part.view(torch.int16)), b0
    assert not bool((gx[B // 2] == CANARY).any())
    assert bool((gx[B - 1] != 0).any()) and bool((y[B - 1] != 0).any())


@pytest.mark.parametrize("B,H,W,C,s,relu6,with_bias", [(2, 14, 14, 96, 1, 1, True), (3, 15, 13, 24, 2, 1, False),
                                                       (2, 7, 7, 960, 1, 0, True)])
def test_autograd_function_equals_the_c_abi_bitwise(B, H, W, C, s, relu6, with_bias):
    """ops.dw_conv3x3 on NCHW-shaped channels_last tensors: no copies in or out, and the very bits of the C-ABI calls."""
    o = ops()
    op = dref.operands("autograd/%s" % ((B, H, W, C, s),), "gaussian", B, H, W, C, s, with_bias)
    want_y = _run_fwd(op, B, H, W, C, s, relu6)
    want_gx = _run_bwd(op, want_y if relu6 else None, B, H, W, C, s, relu6)
    x = op.x.to(DEV).permute(0, 3, 1, 2).requires_grad_(True)
    assert x.is_contiguous(memory_format=torch.channels_last) or H * W == 1
    bias = None if op.bias is None else op.bias.to(DEV)
    y = o.dw_conv3x3(x, op.w9c.to(DEV), bias, s, bool(relu6))
    assert y.shape == (B, C, dref.out_size(H, s), dref.out_size(W, s)) and y.dtype == BF16
    assert y.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(y.detach().permute(0, 2, 3, 1).contiguous().view(torch.int16), want_y.contiguous().view(torch.int16))
    (gx,) = torch.autograd.grad(y, x, op.g.to(DEV).permute(0, 3, 1, 2))
    assert gx.shape == x.shape and gx.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(gx.permute(0, 2, 3, 1).contiguous().view(torch.int16), want_gx.contiguous().view(torch.int16))
    e = torch.zeros(0, C, H, W, dtype=BF16, device=DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ye = o.dw_conv3x3(e, op.w9c.to(DEV), bias, s, bool(relu6))
    assert ye.shape == (0, C, dref.out_size(H, s), dref.out_size(W, s))
    with pytest.raises(ValueError):
        o.dw_conv3x3(x.float(), op.w9c.to(DEV), bias, s, bool(relu6))
    with pytest.raises(ValueError):
        o.dw_conv3x3(x, op.w9c.to(DEV), bias, 3, bool(relu6))


# ------------------------------------------------------------------------------------------------------------- network
def randomised_checkpoint(path, images=None, seed=5, num_classes=1000):
    """A seeded MobileNetV2 state_dict with randomised BatchNorm statistics and affine maps, so that the fold into
    w9c / bias is exercised on every term.  Returns the path.
    images None: statistics drawn around the initial 0 / 1 (mean 0.2 N(0,1), var in [0.6, 1.4], gamma in [0.7, 1.3], beta
      0.2 N(0,1)).  This is the network of the precision comparisons: on the CPU the plain bf16 network (the parent path)
      sits at 0.11 of the bf16 depth bound against its fp32 twin and its input gradient is 21 % off.  Its signal shrinks
      from layer to layer, so the LOGITS are dominated by the biases (their spread over images is at fp32 noise level);
      what depends on the input in that test are the 17 module outputs and the input gradient.
    images given: the statistics of those images (one training-mode pass) perturbed channel by channel, gamma of both
      signs: a network that stays alive through its 52 convolutions, for the learner leg.  Such a network is chaotic in
      bf16 (parent path, CPU: 2.3 x the depth bound, input gradient 113 % off), so it serves no precision comparison."""
    from dl_attack_on_imagenet_amd import zoo
    model = zoo.build_classifier("mobilenet", num_classes=num_classes, seed=seed)
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    gen = torch.Generator().manual_seed(seed + 1)
    r = lambda n: torch.randn(n, generator=gen)
    u = lambda n: torch.rand(n, generator=gen)
    if images is not None:
        for m in bns:
            m.momentum = 1.0
            m.train()
        with torch.no_grad():
            model(images)
        model.eval()
    with torch.no_grad():
        for m in bns:
            n = m.num_features
            if images is None:
                m.weight.copy_(0.7 + 0.6 * u(n))
                m.bias.copy_(0.2 * r(n))
                m.running_mean.copy_(0.2 * r(n))
                m.running_var.copy_(0.6 + 0.8 * u(n))
            else:
                m.running_mean.mul_(1 + 0.2 * r(n)).add_(0.1 * m.running_var.sqrt() * r(n))
                m.running_var.mul_(0.6 + 0.8 * u(n))
                m.weight.copy_((0.7 + 0.6 * u(n)) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1))
                m.bias.copy_(0.3 * r(n))
    torch.save(model[1].state_dict(), path)
    return path


def _networks(tmp_path, num_classes=1000):
    from dl_attack_on_imagenet_amd import zoo
    path = randomised_checkpoint(os.path.join(str(tmp_path), "mobilenet_random_bn.pt"), num_classes=num_classes)
    kw = dict(num_classes=num_classes, seed=5, weights=path, device=DEV)
    ref = zoo.build_classifier("mobilenet", **kw)
    off = zoo.build_classifier("mobilenet", dtype=BF16, channels_last=True, **kw)
    on = zoo.build_classifier("mobilenet", dtype=BF16, channels_last=True, own_depthwise=True, **kw)
    return ref, off, on


def _forward_and_gradient(model, x):
    x = x.clone().requires_grad_(True)
    logits = model(x).float()
    (g,) = torch.autograd.grad(logits.square().sum(), x)
    return logits.detach(), g.detach().float()


def test_mobilenet_on_own_depthwise_kernels(tmp_path, monkeypatch):
    """`own_depthwise=True` on structured images, a checkpoint with randomised BatchNorm statistics: every one of the 17
    modules against the restatement applied to its actual input (gaussian bound), the logits against the fp32 network
    within the bf16 depth bound of 53 layers, the input gradient no further from the fp32 network's than 1.5 x the
    switch-off bf16 network's distance, and no grouped library convolution left.  Recorded on an MI355X: mean |logit error|
    0.00048 off / 0.00047 on against a bound of 0.0043; input-gradient relative error 0.217 off / 0.230 on; every module at
    0.992-0.996 of its elementwise bound (a correctly rounded bf16 result uses all of the 2^-8 |r| term)."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import zoo
    images, _ = structured_images(8, classes=4, seed=3, size=224)
    ref, off, on = _networks(tmp_path)
    x = images.to(DEV)
    blocks = [m for m in on.modules() if isinstance(m, zoo._OwnDepthwise)]
    assert len(blocks) == 17
    seen = []

    def hook(mod, args, out):
        xin = args[0].detach()
        assert xin.dtype == BF16 and xin.is_contiguous(memory_format=torch.channels_last)
        o = dref.dw_fwd(Arith(), xin.permute(0, 2, 3, 1), mod.w9c, mod.bias, mod.stride, 1)
        ratio = dref.gaussian_ratio(out.detach().permute(0, 2, 3, 1), o)
        seen.append((mod.channels, xin.shape[2], mod.stride, ratio))

    handles = [m.register_forward_hook(hook) for m in blocks]
    calls = []
    real_conv2d = F.conv2d

    def counting_conv2d(inp, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
        calls.append(groups)
        return real_conv2d(inp, weight, bias, stride, padding, dilation, groups)

    monkeypatch.setattr(F, "conv2d", counting_conv2d)
    l1, g1 = _forward_and_gradient(on, x.bfloat16())
    grouped_on, dense_on = sum(g > 1 for g in calls), sum(g == 1 for g in calls)
    for h in handles:
        h.remove()
    calls.clear()
    l0, g0 = _forward_and_gradient(off, x.bfloat16())
    grouped_off = sum(g > 1 for g in calls)
    monkeypatch.undo()
    assert (grouped_on, grouped_off, dense_on) == (0, 17, 35), (grouped_on, grouped_off, dense_on)
    assert [(c, h, s) for c, h, s, _ in seen] == dref.MOBILENET_SHAPES_ALL17
    for c, h, s, ratio in seen:
        print("module C=%d H=%d stride %d: max |err| / bound %.3f" % (c, h, s, ratio))
        assert ratio <= 1.0, (c, h, s, ratio)
    lr, gr = _forward_and_gradient(ref, x)
    rms = float(lr.square().mean().sqrt())
    spread = float(lr.std(dim=0).mean())
    e0, e1 = float((l0 - lr).abs().mean()), float((l1 - lr).abs().mean())
    bound = _bf16_depth_bound(53) * rms
    rel = lambda g: float((g - gr).norm() / gr.norm())
    r0, r1 = rel(g0), rel(g1)
    print("logit error vs fp32: switch off %.5f on %.5f, rms %.4f, bound %.5f (spread over images %.4f); input gradient relative "
          "error vs fp32: switch off %.4f on %.4f" % (e0, e1, rms, bound, spread, r0, r1))
    assert float(gr.abs().max()) > 0 and float(g1.abs().max()) > 0      # the input gradient is what depends on the input
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all()
    assert e1 <= bound, (e0, e1, rms)
    assert g1.shape == x.shape
    assert r1 <= 1.5 * r0, (r0, r1)


def test_switch_off_is_the_parent_network(tmp_path):
    """own_depthwise=False and a network built without the argument: the same modules, the same state_dict."""
    from dl_attack_on_imagenet_amd import zoo
    kw = dict(num_classes=10, seed=5, device=DEV, dtype=BF16, channels_last=True)
    a = zoo.build_classifier("mobilenet", **kw)
    b = zoo.build_classifier("mobilenet", own_depthwise=False, **kw)
    assert [type(m) for m in a.modules()] == [type(m) for m in b.modules()]
    assert not any(isinstance(m, zoo._OwnDepthwise) for m in b.modules())
    assert sorted(a.state_dict()) == sorted(b.state_dict())


def test_dw3x3_is_bitwise_across_processes():
    """Two fresh child processes, one after the other (the second only if the first exited 0), each under `timeout`:
    byte-identical y and gx for three shapes."""
    child = os.path.join(ROOT, "tests", "depthwise_child.py")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
    outs = []
    for _ in range(2):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, child], env=env, capture_output=True, text=True,
                           timeout=270, cwd=ROOT)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("hash ")]
        assert len(lines) == 6, r.stdout[-2000:]               # three shapes, y and gx
        outs.append(lines)
    for a, b in zip(*outs):
        assert a == b, (a, b)


def test_learner_steps_against_mobilenet_reported(tmp_path):
    """Reported leg, sanity bounds only: 20 learner steps (bf16 streams, 32 structured images, K = 10) against MobileNetV2
    with the switch off and on.  All values finite, at least one image fooled on each side; both counts are printed."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import engine, zoo
    images, labels = structured_images(32, classes=4, seed=7, noise=0.15)
    path = randomised_checkpoint(os.path.join(str(tmp_path), "mobilenet_random_bn.pt"), images[:8], num_classes=4)
    plain = zoo.build_classifier("mobilenet", num_classes=4, seed=5, weights=path, device=DEV)
    margins, pred = zoo.fit_centroid_head(plain, images, labels, 4, DEV, target_margin=2.0)
    assert bool((pred.cpu() == labels).all())
    path = os.path.join(str(tmp_path), "mobilenet_fitted.pt")
    torch.save(plain[-1].state_dict(), path)
    x = images.to(DEV).bfloat16().contiguous()
    gen = torch.Generator().manual_seed(0)
    n, k, eps = 32, 10, EPS_LEARNER
    d0 = -1 + 2 * torch.rand(3, 224, 224, k, generator=gen)
    v0 = ops().l1ball_project_(torch.rand(n, k, generator=gen).to(DEV), eps).cpu()
    index = torch.arange(n, device=DEV)
    fooled = {}
    for name, own in (("off", False), ("on", True)):
        model = zoo.build_classifier("mobilenet", num_classes=4, seed=5, weights=path, device=DEV, dtype=BF16,
                                     channels_last=True, own_depthwise=own)
        learner = engine.DictionaryLearner(d0.clone().to(DEV), v0.clone().to(DEV), eps, 0.01, "logits", False, 50.0)
        last = None
        for _ in range(20):
            ls, fl = learner.step(model, x, index)
            last = (float(ls), int(fl))
        assert torch.isfinite(learner.d).all() and torch.isfinite(learner.v).all() and last[0] == last[0]
        fooled[name] = last[1]
    print("fooled after 20 steps of 32 images: switch off %d, on %d" % (fooled["off"], fooled["on"]))
    assert fooled["off"] >= 1 and fooled["on"] >= 1, fooled
