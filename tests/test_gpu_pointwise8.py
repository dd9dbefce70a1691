"""GPU: the narrow-channel pointwise kernels (adil_pw8_fwd / adil_pw8_bwd, csrc/adil_pointwise8.hip) through the C ABI
against the fp64 restatement of tests/pointwise8_reference.py — bit for bit on the exact legs, under the derived elementwise
bound on the gaussian leg — and the MobileNetV2 that runs its 34 1x1 layers on them (`own_pointwise=True`)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import pointwise8_reference as pref
from classifier_reference import BF16, CANARY, Arith

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PAD = 5                          # canary rows behind every output
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


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _run_fwd(x, w, scale, shift, res, act):
    """Device tensors in, y [M][N] out; canary rows behind y."""
    o, lib = ops(), _lib()
    M, K, N = x.shape[0], x.shape[1], w.shape[0]
    y = torch.full((M + PAD, N), CANARY, dtype=BF16, device=DEV)
    assert lib.adil_pw8_fwd(o._ptr(x), o._ptr(w), o._ptr(scale), o._ptr(shift), o._ptr(res), o._ptr(y), M, K, N, act,
                            o._stream()) == 0
    torch.cuda.synchronize()
    assert bool((y[M:] == CANARY).all()), "forward wrote past the end of y"
    return y[:M]


def _run_bwd(g, y, scale, wt, act):
    o, lib = ops(), _lib()
    M, N, K = g.shape[0], g.shape[1], wt.shape[0]
    gx = torch.full((M + PAD, K), CANARY, dtype=BF16, device=DEV)
    assert lib.adil_pw8_bwd(o._ptr(g), o._ptr(y), o._ptr(scale), o._ptr(wt), o._ptr(gx), M, K, N, act, o._stream()) == 0
    torch.cuda.synchronize()
    assert bool((gx[M:] == CANARY).all()), "gradient wrote past the end of gx"
    return gx[:M]


def _fwd(op, res, act):
    return _run_fwd(_dev(op.x), _dev(op.w), _dev(op.scale), _dev(op.shift), _dev(res), act)


def _bwd(op, y, act):
    return _run_bwd(_dev(op.g), _dev(y), _dev(op.scale), _dev(op.wt), act)


def _exact_references(name, leg, M, K, N, with_res, a):
    """Operands and fp64 references of one exact-leg comparison; every premise is asserted on the reference alone."""
    op = pref.operands(name, leg, M, K, N, with_res and not a)
    res = None if a else op.res
    ref = pref.pw8_fwd(Arith(), op.x, op.w, op.scale, op.shift, res, a)
    worst, inexact = pref.assert_premise(name + "/fwd", ref, leg)
    y = None
    if a:
        y = pref.mask_source(name, leg, pref.finish(Arith(), ref))
        pref.assert_branches(name + "/fwd", ref.pre)
        pref.assert_branches(name + "/mask", y.double())
    refb = pref.pw8_bwd(Arith(), op.g, y, op.scale, op.wt, a)
    worstb, inexactb = pref.assert_premise(name + "/bwd", refb, leg)
    print(name, "sum |terms| in quanta fwd %.0f bwd %.0f, outputs that need rounding fwd %.2f bwd %.2f" % (worst, worstb, inexact,
                                                                                                         inexactb))
    return op, res, y, ref, refb


@pytest.mark.parametrize("row", pref.ROWS, ids=str)
def test_pw8_against_the_fp64_restatement(row):
    """Forward and input gradient of one row on the exact legs (clamp set when the row has a ReLU6, rounding set always,
    with act = 0 and the row's residual) and on the gaussian leg.  Row names and operands are those of
    tests/test_pointwise8_cpu.py, where the emulation passes them."""
    M, K, N, act, with_res = row
    for leg, a in ([("clamp", 1)] if act else []) + [("rounding", 0)]:
        name = "p8/%s/%s" % (row, leg)
        op, res, y, ref, refb = _exact_references(name, leg, M, K, N, with_res, a)
        pref.compare_exact(name + "/fwd", _fwd(op, res, a), ref)
        pref.compare_exact(name + "/bwd", _bwd(op, y, a), refb)
    name = "p8/%s/gaussian" % (row,)
    op = pref.operands(name, "gaussian", M, K, N, with_res)
    ref = pref.pw8_fwd(Arith(), op.x, op.w, op.scale, op.shift, op.res, act)
    got = _fwd(op, op.res, act)
    rf = pref.gaussian_ratio(got.cpu(), ref)
    y = got.cpu() if act else None                       # the mask source: the kernel's own stored output, on both sides
    refb = pref.pw8_bwd(Arith(), op.g, y, op.scale, op.wt, act)
    rb = pref.gaussian_ratio(_bwd(op, y, act).cpu(), refb)
    print(name, "max |err| / bound: fwd %.3f bwd %.3f" % (rf, rb))
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)


def _in_nan(t):
    """The same values as a view into a larger buffer of bf16 NaN: 64 NaN directly in front of and behind the operand."""
    t = t.to(DEV).contiguous()
    buf = torch.full((t.numel() + 128,), float("nan"), dtype=BF16, device=DEV)
    buf[64:64 + t.numel()] = t.reshape(-1)
    v = buf[64:64 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 0 and bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all())
    return v


@pytest.mark.parametrize("M,K,N", pref.NAN_ROWS)
def test_pw8_reads_nothing_outside_its_operands(M, K, N):
    """x, w, g and wt surrounded by NaN: the K tail (K % 16 = 8, K % 64 != 0) and the N tail (N % 32 = 8) are clipped and
    zero-filled, not read from the neighbouring row or from behind the operand.  Exact legs: the result equals the
    restatement (and with it the result of the plain operands) bit for bit and holds no NaN."""
    row = (M, K, N, 1, False)
    for leg, a in (("clamp", 1), ("rounding", 0)):
        name = "p8/%s/%s" % (row, leg)
        op, res, y, ref, refb = _exact_references(name, leg, M, K, N, False, a)
        plain_y, plain_gx = _fwd(op, None, a), _bwd(op, y, a)
        got_y = _run_fwd(_in_nan(op.x), _in_nan(op.w), _dev(op.scale), _dev(op.shift), None, a)
        got_gx = _run_bwd(_in_nan(op.g), _dev(y), _dev(op.scale), _in_nan(op.wt), a)
        assert not bool(torch.isnan(got_y).any()) and not bool(torch.isnan(got_gx).any())
        assert torch.equal(got_y.view(torch.int16), plain_y.view(torch.int16))
        assert torch.equal(got_gx.view(torch.int16), plain_gx.view(torch.int16))
        pref.compare_exact(name + "/fwd", got_y, ref)
        pref.compare_exact(name + "/bwd", got_gx, refb)


def test_pw8_refuses_and_leaves_outputs_untouched():
    """K = 12, N = 20, K = 2056, M = 0, res with act 1, act 2, NULL x, NULL y with act 1, a misaligned pointer: ADIL_EINVAL,
    canaries intact."""
    o, lib = ops(), _lib()
    big = torch.zeros(64 * 2064, dtype=BF16, device=DEV)
    tab = torch.zeros(2064, dtype=torch.float32, device=DEV)
    out = torch.full((64 * 2064,), CANARY, dtype=BF16, device=DEV)
    P, S = o._ptr, o._stream

    def fwd(x, w, sc, sh, res, y, M, K, N, act):
        return lib.adil_pw8_fwd(x, w, sc, sh, res, y, M, K, N, act, S())

    def bwd(g, y, sc, wt, gx, M, K, N, act):
        return lib.adil_pw8_bwd(g, y, sc, wt, gx, M, K, N, act, S())

    for (M, K, N, act) in [(64, 12, 16, 0), (64, 16, 20, 0), (64, 2056, 16, 0), (64, 16, 2056, 1), (0, 16, 16, 1), (64, 16, 16, 2),
                           (64, 16, 16, -1), (64, 0, 16, 0), (64, 4, 8, 1)]:
        assert fwd(P(big), P(big), P(tab), P(tab), None, P(out), M, K, N, act) == EINVAL, (M, K, N, act)
        assert bwd(P(big), P(big), P(tab), P(big), P(out), M, K, N, act) == EINVAL, (M, K, N, act)
    assert fwd(P(big), P(big), P(tab), P(tab), P(big), P(out), 64, 16, 16, 1) == EINVAL                 # res with act 1
    assert fwd(None, P(big), P(tab), P(tab), None, P(out), 64, 16, 16, 0) == EINVAL                     # NULL x
    assert fwd(P(big), None, P(tab), P(tab), None, P(out), 64, 16, 16, 0) == EINVAL
    assert fwd(P(big), P(big), None, P(tab), None, P(out), 64, 16, 16, 0) == EINVAL
    assert fwd(P(big), P(big), P(tab), None, None, P(out), 64, 16, 16, 0) == EINVAL
    assert fwd(P(big), P(big), P(tab), P(tab), None, None, 64, 16, 16, 0) == EINVAL
    assert bwd(None, P(big), P(tab), P(big), P(out), 64, 16, 16, 1) == EINVAL
    assert bwd(P(big), None, P(tab), P(big), P(out), 64, 16, 16, 1) == EINVAL                           # act 1 needs y
    assert bwd(P(big), P(big), None, P(big), P(out), 64, 16, 16, 1) == EINVAL
    assert bwd(P(big), P(big), P(tab), None, P(out), 64, 16, 16, 1) == EINVAL
    assert bwd(P(big), P(big), P(tab), P(big), None, 64, 16, 16, 1) == EINVAL
    assert fwd(P(big[4:]), P(big), P(tab), P(tab), None, P(out), 64, 16, 16, 0) == EINVAL               # misaligned x
    assert fwd(P(big), P(big), P(tab), P(tab), None, P(out[4:]), 64, 16, 16, 0) == EINVAL               # misaligned y
    assert fwd(P(big), P(big), P(tab[1:]), P(tab), None, P(out), 64, 16, 16, 0) == EINVAL
    assert fwd(P(big), P(big), P(tab), P(tab), P(big[4:]), P(out), 64, 16, 16, 0) == EINVAL
    assert bwd(P(big), P(big), P(tab), P(big[4:]), P(out), 64, 16, 16, 1) == EINVAL                     # misaligned wt
    assert bwd(P(big), P(big[4:]), P(tab), P(big), P(out), 64, 16, 16, 1) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    # the accepted forms of the optional pointers: res NULL, y NULL (even misaligned: it is not read) without a ReLU6
    assert fwd(P(big), P(big), P(tab), P(tab), None, P(out), 64, 16, 16, 1) == 0
    assert bwd(P(big), None, P(tab), P(big), P(out), 64, 16, 16, 0) == 0
    torch.cuda.synchronize()
    assert bool((out[:64 * 16] == 0).all()) and bool((out[64 * 16:] == CANARY).all())


def test_pw8_beyond_2_31_elements():
    """K = 16, N = 96 (the 16 -> 96 expansion) at M = 22,400,037 pixels: y, g and the mask source hold 2.15e9 elements
    (offsets pass 2^31, and 2^32 bytes).  Exact leg (clamp set, ReLU6): the first tile, the last (partial) tile and the rows
    straddling element 2^31 against the restatement, bit for bit, forward and gradient."""
    _need(16)
    M, K, N = 22_400_037, 16, 96
    assert M * N > 2 ** 31 and M % 128 != 0
    cut = 2 ** 31 // N
    windows = [(0, 256), (cut - 128, cut + 128), (M - 256, M)]
    op = pref.operands("big", "clamp", 1, K, N)
    w, wt, scale, shift = _dev(op.w), _dev(op.wt), _dev(op.scale), _dev(op.shift)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)

    def fill(t, lo, hi):
        step = 1 << 21
        for m0 in range(0, t.shape[0], step):
            part = t[m0:m0 + step]
            part.copy_(torch.randint(lo, hi + 1, part.shape, generator=gen, device=DEV, dtype=torch.int8))
        return t

    x = fill(torch.empty((M, K), dtype=BF16, device=DEV), -2, 2)
    y = _run_fwd(x, w, scale, shift, None, 1)
    for lo, hi in windows:
        ref = pref.pw8_fwd(Arith(), x[lo:hi].cpu(), op.w, op.scale, op.shift, None, 1)
        pref.assert_premise("big/fwd/%d" % lo, ref, "clamp")
        pref.assert_branches("big/fwd/%d" % lo, ref.pre)
        pref.compare_exact("big/fwd/%d" % lo, y[lo:hi], ref)
    assert not bool((y[M // 2 - 4096:M // 2 + 4096] == CANARY).any())
    del x
    g = fill(torch.empty((M, N), dtype=BF16, device=DEV), -3, 3)
    gx = _run_bwd(g, y, scale, wt, 1)
    for lo, hi in windows:
        refb = pref.pw8_bwd(Arith(), g[lo:hi].cpu(), y[lo:hi].cpu(), op.scale, op.wt, 1)
        pref.assert_premise("big/bwd/%d" % lo, refb, "clamp")
        pref.compare_exact("big/bwd/%d" % lo, gx[lo:hi], refb)
    assert bool((gx[M - 256:] != 0).any()) and not bool((gx[M // 2 - 4096:M // 2 + 4096] == CANARY).any())


AUTOGRAD_ROWS = [(2, 14, 14, 96, 576, 1, False), (3, 7, 5, 144, 24, 0, True), (2, 9, 11, 24, 40, 0, False)]


def _nchw(t, b, h, w):
    return t.to(DEV).reshape(b, h, w, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("b,h,w,k,n,act,with_res", AUTOGRAD_ROWS)
def test_autograd_function_equals_the_c_abi_bitwise(b, h, w, k, n, act, with_res):
    """ops.pw8_conv on NCHW-shaped channels_last tensors: no copies in or out, the very bits of the C-ABI calls, and the
    residual input's gradient is the incoming gradient."""
    o = ops()
    op = pref.operands("autograd/%s" % ((b, h, w, k, n),), "gaussian", b * h * w, k, n, with_res)
    want_y = _fwd(op, op.res, act)
    want_gx = _bwd(op, want_y if act else None, act)
    x = _nchw(op.x, b, h, w).requires_grad_(True)
    res = _nchw(op.res, b, h, w).requires_grad_(True) if with_res else None
    args = (_dev(op.w), _dev(op.wt), _dev(op.scale), _dev(op.shift))
    y = o.pw8_conv(x, *args, res, bool(act))
    assert y.shape == (b, n, h, w) and y.dtype == BF16 and y.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(y.detach().permute(0, 2, 3, 1).reshape(-1, n).view(torch.int16), want_y.view(torch.int16))
    g = _nchw(op.g, b, h, w)
    grads = torch.autograd.grad(y, (x, res) if with_res else (x,), g)
    gx = grads[0]
    assert gx.shape == x.shape and gx.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(gx.permute(0, 2, 3, 1).reshape(-1, k).view(torch.int16), want_gx.view(torch.int16))
    if with_res:
        assert grads[1].shape == res.shape and torch.equal(grads[1].contiguous().view(torch.int16), g.contiguous().view(torch.int16))
        with pytest.raises(ValueError):
            o.pw8_conv(x, *args, res, True)
    with pytest.raises(ValueError):
        o.pw8_conv(x.float(), *args, None, bool(act))
    with pytest.raises(ValueError):
        o.pw8_conv(x[:, :k - 4], *args, None, bool(act))
    with pytest.raises(ValueError):
        o.pw8_conv(x, args[0], args[1], args[2].double(), args[3], None, bool(act))


def test_pw8_in_a_captured_graph():
    """One layer's forward + input gradient captured in a graph and replayed (on fresh inputs copied into the captured
    buffers) equals the eager result bit for bit: the calls launch on the capturing stream and neither synchronise nor
    allocate outside the allocator."""
    o = ops()
    b, h, w, k, n = 4, 14, 14, 96, 576
    op = pref.operands("graph", "gaussian", b * h * w, k, n)
    op2 = pref.operands("graph/2", "gaussian", b * h * w, k, n)
    args = (_dev(op.w), _dev(op.wt), _dev(op.scale), _dev(op.shift))

    def run(x, g):
        y = o.pw8_conv(x, *args, None, True)
        (gx,) = torch.autograd.grad(y, x, g)
        return y, gx

    eager = [tuple(t.detach().clone() for t in run(_nchw(q.x, b, h, w).requires_grad_(True), _nchw(q.g, b, h, w))) for q in (op, op2)]
    xs = _nchw(op.x, b, h, w).clone(memory_format=torch.preserve_format).requires_grad_(True)
    gs = _nchw(op.g, b, h, w).clone(memory_format=torch.preserve_format)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(xs, gs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys, gxs = run(xs, gs)
    for q, (want_y, want_gx) in zip((op, op2), eager):
        with torch.no_grad():
            xs.copy_(_nchw(q.x, b, h, w))
            gs.copy_(_nchw(q.g, b, h, w))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ys.detach().contiguous().view(torch.int16), want_y.contiguous().view(torch.int16))
        assert torch.equal(gxs.contiguous().view(torch.int16), want_gx.contiguous().view(torch.int16))


# ------------------------------------------------------------------------------------------------------------- network
def randomised_checkpoint(path, images=None, seed=5, num_classes=1000):
    """The recipe of tests/test_gpu_depthwise.py, restated: a seeded MobileNetV2 state_dict with randomised BatchNorm
    statistics and affine maps, so that every term of the epilogue tables is exercised.
    images None: statistics drawn around the initial 0 / 1 (mean 0.2 N(0,1), var in [0.6, 1.4], gamma in [0.7, 1.3], beta
      0.2 N(0,1)): the network of the precision comparisons (its logits are dominated by the biases; what depends on the
      input are the module outputs and the input gradient).
    images given: the statistics of those images (one training-mode pass) perturbed channel by channel, gamma of both
      signs: a network that stays alive through its 52 convolutions, for the learner leg (chaotic in bf16: it serves no
      precision comparison)."""
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


def _forward_and_gradient(model, x):
    x = x.clone().requires_grad_(True)
    logits = model(x).float()
    (g,) = torch.autograd.grad(logits.square().sum(), x)
    return logits.detach(), g.detach().float()


class _Calls:
    """Counts the library convolutions (grouped / dense) and BatchNorm calls of a forward pass."""

    def __init__(self, monkeypatch):
        self.groups, self.bn = [], 0
        real_conv2d, real_bn = F.conv2d, F.batch_norm

        def conv2d(inp, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
            self.groups.append(groups)
            return real_conv2d(inp, weight, bias, stride, padding, dilation, groups)

        def batch_norm(*args, **kw):
            self.bn += 1
            return real_bn(*args, **kw)

        monkeypatch.setattr(F, "conv2d", conv2d)
        monkeypatch.setattr(F, "batch_norm", batch_norm)

    def take(self):
        out = (sum(g > 1 for g in self.groups), sum(g == 1 for g in self.groups), self.bn)
        self.groups, self.bn = [], 0
        return out


def test_mobilenet_on_own_pointwise_kernels(tmp_path, monkeypatch):
    """`own_pointwise=True` on 8 structured images at 224 x 224, a checkpoint with randomised BatchNorm statistics: each of
    the 34 rewritten layers against the restatement applied to its actual input (gaussian bound, ratio printed), the
    library calls that are left (both switches: the 3 -> 32 first convolution and its BatchNorm alone), the logits against
    the fp32 network within the bf16 depth bound of 53 layers, and the input gradient no further from the fp32 network's
    than 1.5 x the distance of the plain bf16 network (the parent path).  Recorded on an MI355X: every layer at 0.88-0.995 of
    its elementwise bound (a correctly rounded bf16 result uses all of the 2^-8 |r| term); mean |logit error| 0.00048 off /
    0.00037 own_pointwise / 0.00036 both against a bound of 0.0043; input-gradient relative error 0.217 / 0.204 / 0.181."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import zoo
    images, _ = structured_images(8, classes=4, seed=3, size=224)
    path = randomised_checkpoint(os.path.join(str(tmp_path), "mobilenet_random_bn.pt"))
    kw = dict(num_classes=1000, seed=5, weights=path, device=DEV)
    ref = zoo.build_classifier("mobilenet", **kw)
    kw.update(dtype=BF16, channels_last=True)
    off = zoo.build_classifier("mobilenet", **kw)
    pw = zoo.build_classifier("mobilenet", own_pointwise=True, **kw)
    both = zoo.build_classifier("mobilenet", own_pointwise=True, own_depthwise=True, **kw)
    x = images.to(DEV)
    seen, held = [], {}

    def restate(mod, conv, xin, res, out, act):
        assert xin.dtype == BF16 and xin.is_contiguous(memory_format=torch.channels_last)
        flat = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1])
        o = pref.pw8_fwd(Arith(), flat(xin), conv.weight.detach().reshape(mod.cout, mod.cin), mod.scale, mod.shift,
                         None if res is None else flat(res), act)
        seen.append((mod.cin, mod.cout, xin.shape[2], act, res is not None, pref.gaussian_ratio(flat(out), o)))

    handles = []
    for m in both.modules():
        if isinstance(m, zoo._OwnPointwise):
            handles.append(m.register_forward_hook(lambda mod, args, out: restate(mod, mod[0], args[0], None, out, 1)))
        elif isinstance(m, zoo._OwnInvertedResidual):
            # the projection's own input is the output of the layer in front of it
            handles.append(m.conv[-3].register_forward_hook(lambda mod, args, out, blk=m: held.__setitem__(blk, out)))
            handles.append(m.register_forward_hook(lambda mod, args, out: restate(
                mod, mod.conv[-2], held.pop(mod), args[0] if mod.use_res else None, out, 0)))
    assert len(handles) == 17 + 2 * 17
    calls = _Calls(monkeypatch)
    l2, g2 = _forward_and_gradient(both, x.bfloat16())
    n_both = calls.take()
    for h in handles:
        h.remove()
    l1, g1 = _forward_and_gradient(pw, x.bfloat16())
    n_pw = calls.take()
    l0, g0 = _forward_and_gradient(off, x.bfloat16())
    n_off = calls.take()
    monkeypatch.undo()
    print("library calls (grouped conv, dense conv, BatchNorm): off %s, own_pointwise %s, both switches %s" % (n_off, n_pw, n_both))
    assert n_off == (17, 35, 52) and n_both == (0, 1, 1) and n_pw[:2] == (17, 1) and n_pw[2] == 18
    assert [s[:5] for s in seen] == pref.MOBILENET_LAYERS_ALL34
    for k, n, h, act, res, ratio in seen:
        print("layer %4d -> %4d at %3d x %3d act %d res %d: max |err| / bound %.3f" % (k, n, h, h, act, res, ratio))
        assert ratio <= 1.0, (k, n, h, act, res, ratio)
    lr, gr = _forward_and_gradient(ref, x)
    rms = float(lr.square().mean().sqrt())
    bound = _bf16_depth_bound(53) * rms
    rel = lambda g: float((g - gr).norm() / gr.norm())
    e0, e1, e2 = (float((l - lr).abs().mean()) for l in (l0, l1, l2))
    r0, r1, r2 = rel(g0), rel(g1), rel(g2)
    print("logit error vs fp32: off %.5f own_pointwise %.5f both %.5f, rms %.4f, bound %.5f; input gradient relative error vs "
          "fp32: off %.4f own_pointwise %.4f both %.4f" % (e0, e1, e2, rms, bound, r0, r1, r2))
    assert float(gr.abs().max()) > 0 and float(g1.abs().max()) > 0 and float(g2.abs().max()) > 0
    for l, g in ((l1, g1), (l2, g2)):
        assert torch.isfinite(l).all() and torch.isfinite(g).all() and g.shape == x.shape
    assert e1 <= bound and e2 <= bound, (e0, e1, e2, rms)
    assert r1 <= 1.5 * r0 and r2 <= 1.5 * r0, (r0, r1, r2)


def test_pw8_is_bitwise_across_processes():
    """Two fresh child processes, one after the other (the second only if the first exited 0), each under `timeout`:
    byte-identical y and gx for three rows."""
    child = os.path.join(ROOT, "tests", "pointwise8_child.py")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
    outs = []
    for _ in range(2):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, child], env=env, capture_output=True, text=True,
                           timeout=270, cwd=ROOT)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("hash ")]
        assert len(lines) == 6, r.stdout[-2000:]               # three rows, y and gx
        outs.append(lines)
    for a, b in zip(*outs):
        assert a == b, (a, b)


def test_learner_steps_against_mobilenet_reported(tmp_path):
    """Reported leg, sanity bounds only: 20 learner steps (bf16 streams, 32 structured images, K = 10) against MobileNetV2
    with both switches on.  All values finite, at least one image fooled; the count is printed."""
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
    model = zoo.build_classifier("mobilenet", num_classes=4, seed=5, weights=path, device=DEV, dtype=BF16, channels_last=True,
                                 own_depthwise=True, own_pointwise=True)
    learner = engine.DictionaryLearner(d0.clone().to(DEV), v0.clone().to(DEV), eps, 0.01, "logits", False, 50.0)
    last = None
    for _ in range(20):
        ls, fl = learner.step(model, x, index)
        last = (float(ls), int(fl))
    assert torch.isfinite(learner.d).all() and torch.isfinite(learner.v).all() and last[0] == last[0]
    print("fooled after 20 steps of 32 images, both switches on: %d (loss %.4f)" % (last[1], last[0]))
    assert last[1] >= 1, last
