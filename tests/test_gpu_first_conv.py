"""GPU: the first-convolution kernels (adil_first3x3_fwd / adil_first3x3_bwd, csrc/adil_first_conv.hip) through the C ABI
against the fp64 restatement of tests/first_conv_reference.py — bit for bit on the exact legs, under the derived elementwise
bound on the gaussian leg — and the MobileNetV2 that runs its first layer on them (`own_first_conv=True`), alone and with
`own_depthwise` and `own_pointwise`, when no library convolution and no library BatchNorm is left."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import first_conv_reference as fref
from classifier_reference import BF16, CANARY, F32, Arith

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PAD = 256                        # canary elements in front of and behind every output
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


def _code(dtype):
    return {F32: 0, BF16: 1}[dtype]


def _guarded(shape, dtype):
    """An output of `shape` inside a canary-filled buffer; returns (buffer, view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), CANARY, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n].view(shape)


def _intact(buf):
    return bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all())


def _run_fwd(x, wf, mean, inv_std, scale, shift, relu6):
    """Device tensors in (x [B][3][H][W], wf the packed weight), y [B][OH][OW][32] out; canaries around y."""
    o, lib = ops(), _lib()
    B, _, H, W = x.shape
    OH, OW = fref.out_grid(H, W)
    buf, y = _guarded((B, OH, OW, 32), BF16)
    assert lib.adil_first3x3_fwd(o._ptr(x), _code(x.dtype), o._ptr(wf), *mean, *inv_std, o._ptr(scale), o._ptr(shift),
                                 o._ptr(y), B, H, W, relu6, o._stream()) == 0
    torch.cuda.synchronize()
    assert _intact(buf), "forward wrote outside y"
    return y


def _run_bwd(g, y, scale, wb, inv_std, H, W, relu6, dtype):
    o, lib = ops(), _lib()
    B = g.shape[0]
    buf, gx = _guarded((B, 3, H, W), dtype)
    assert lib.adil_first3x3_bwd(o._ptr(g), o._ptr(y), o._ptr(scale), o._ptr(wb), *inv_std, o._ptr(gx), _code(dtype), B, H, W,
                                 relu6, o._stream()) == 0
    torch.cuda.synchronize()
    assert _intact(buf), "gradient wrote outside gx"
    return gx


def _fwd(op, relu6, wrap=_dev):
    return _run_fwd(wrap(op.x), wrap(fref.pack_fwd(op.w)), op.mean, op.inv_std, _dev(op.scale), _dev(op.shift), relu6)


def _bwd(op, y, H, W, relu6, dtype, wrap=_dev):
    return _run_bwd(wrap(op.g), None if y is None else wrap(y), _dev(op.scale), wrap(fref.pack_bwd(op.w)), op.inv_std, H, W,
                    relu6, dtype)


@pytest.mark.parametrize("row", fref.ROWS, ids=str)
def test_first_conv_against_the_fp64_restatement(row):
    """Forward and input gradient of one row on the exact legs (clamp set when the row has a ReLU6, rounding set always)
    and on the gaussian leg.  Row names and operands are those of tests/test_first_conv_cpu.py, where the emulation passes
    them."""
    B, H, W, dtype, relu6 = row
    for leg in fref.exact_legs(relu6):
        name = fref.row_name(row, leg)
        a = 1 if leg == "clamp" else 0
        op, y, ref, refb = fref.exact_references(name, leg, B, H, W, dtype)
        fref.compare_exact(name + "/fwd", _fwd(op, a), ref)
        fref.compare_exact(name + "/bwd", _bwd(op, y, H, W, a, dtype), refb)
    name = fref.row_name(row, "gaussian")
    op = fref.operands(name, "gaussian", B, H, W, dtype)
    ref = fref.first_fwd(Arith(), op.x, op.w, op.mean, op.inv_std, op.scale, op.shift, relu6)
    got = _fwd(op, relu6)
    rf = fref.gaussian_ratio(got.cpu(), ref)
    y = got.cpu() if relu6 else None                     # the mask source: the kernel's own stored output, on both sides
    refb = fref.first_bwd(Arith(), op.g, y, op.scale, op.w, op.inv_std, H, W, relu6, dtype)
    rb = fref.gaussian_ratio(_bwd(op, y, H, W, relu6, dtype).cpu(), refb)
    print(name, "max |err| / bound: fwd %.3f bwd %.3f" % (rf, rb))
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)


def _in_nan(t):
    """The same values as a view into a larger buffer of NaN: 64 NaN directly in front of and behind the operand."""
    t = t.to(DEV).contiguous()
    buf = torch.full((t.numel() + 128,), float("nan"), dtype=t.dtype, device=DEV)
    buf[64:64 + t.numel()] = t.reshape(-1)
    v = buf[64:64 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 0 and bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all())
    return v


def _same_bits(a, b):
    view = torch.int16 if a.dtype == BF16 else torch.int32
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


@pytest.mark.parametrize("B,H,W", fref.NAN_ROWS)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_first_conv_reads_nothing_outside_its_operands(B, H, W, dtype):
    """x, g, y and the packed weights surrounded by NaN, the outputs by canaries: the border taps and the tile tails are
    predicated, not read from the neighbouring row or from behind the operand.  Exact legs: the result equals the
    restatement (and with it the result of the plain operands) bit for bit and holds no NaN."""
    row = (B, H, W, dtype, 1)
    for leg in fref.exact_legs(1):
        name = fref.row_name(row, leg)
        a = 1 if leg == "clamp" else 0
        op, y, ref, refb = fref.exact_references(name, leg, B, H, W, dtype)
        plain_y, plain_gx = _fwd(op, a), _bwd(op, y, H, W, a, dtype)
        got_y, got_gx = _fwd(op, a, _in_nan), _bwd(op, y, H, W, a, dtype, _in_nan)
        assert bool(torch.isfinite(got_y.float()).all()) and bool(torch.isfinite(got_gx.float()).all())
        assert _same_bits(got_y, plain_y) and _same_bits(got_gx, plain_gx)
        fref.compare_exact(name + "/fwd", got_y, ref)
        fref.compare_exact(name + "/bwd", got_gx, refb)


def test_first_conv_refuses_and_leaves_outputs_untouched():
    """A NULL mandatory pointer, a non-positive size, a dtype code outside the two, relu6 outside {0, 1}, a misaligned
    pointer: ADIL_EINVAL, canaries intact."""
    o, lib = ops(), _lib()
    big = torch.zeros(1 << 16, dtype=BF16, device=DEV)
    tab = torch.zeros(64, dtype=F32, device=DEV)
    out = torch.full((1 << 16,), CANARY, dtype=BF16, device=DEV)
    P, S = o._ptr, o._stream
    nm = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)

    def fwd(x, dt, w, sc, sh, y, B, H, W, r):
        return lib.adil_first3x3_fwd(x, dt, w, *nm, sc, sh, y, B, H, W, r, S())

    def bwd(g, y, sc, w, gx, dt, B, H, W, r):
        return lib.adil_first3x3_bwd(g, y, sc, w, *nm[3:], gx, dt, B, H, W, r, S())

    for (B, H, W, dt, r) in [(0, 8, 8, 1, 1), (-1, 8, 8, 1, 1), (2, 0, 8, 1, 1), (2, 8, 0, 1, 1), (2, 8, -8, 1, 0), (2, 8, 8, 2, 1),
                             (2, 8, 8, -1, 1), (2, 8, 8, 1, 2), (2, 8, 8, 1, -1), (65536, 1, 1, 1, 1)]:
        assert fwd(P(big), dt, P(big), P(tab), P(tab), P(out), B, H, W, r) == EINVAL, (B, H, W, dt, r)
        assert bwd(P(big), P(big), P(tab), P(big), P(out), dt, B, H, W, r) == EINVAL, (B, H, W, dt, r)
    a = (P(big), 1, P(big), P(tab), P(tab), P(out))
    for i in (0, 2, 3, 4, 5):                                          # each NULL mandatory pointer of the forward
        assert fwd(*(None if j == i else v for j, v in enumerate(a)), 2, 8, 8, 1) == EINVAL, i
    a = (P(big), P(big), P(tab), P(big), P(out))
    for i in range(5):                                                 # and of the gradient (y: mandatory with relu6)
        assert bwd(*(None if j == i else v for j, v in enumerate(a)), 1, 2, 8, 8, 1) == EINVAL, i
    assert fwd(P(big), 1, P(big[4:]), P(tab), P(tab), P(out), 2, 8, 8, 1) == EINVAL                     # misaligned w_fwd
    assert fwd(P(big), 1, P(big), P(tab), P(tab), P(out[4:]), 2, 8, 8, 1) == EINVAL                     # misaligned y
    assert fwd(P(big[1:]), 0, P(big), P(tab), P(tab), P(out), 2, 8, 8, 1) == EINVAL                     # fp32 x at 2 bytes
    assert bwd(P(big[4:]), P(big), P(tab), P(big), P(out), 1, 2, 8, 8, 1) == EINVAL                     # misaligned g
    assert bwd(P(big), P(big[4:]), P(tab), P(big), P(out), 1, 2, 8, 8, 1) == EINVAL                     # misaligned y
    assert bwd(P(big), P(big), P(tab), P(big[4:]), P(out), 1, 2, 8, 8, 1) == EINVAL                     # misaligned w_bwd
    assert bwd(P(big), P(big), P(tab), P(big), P(out[1:]), 0, 2, 8, 8, 1) == EINVAL                     # fp32 gx at 2 bytes
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    # the accepted forms: x and gx on any element boundary, y NULL (even misaligned: it is not read) without a ReLU6
    assert fwd(P(big[1:]), 1, P(big), P(tab), P(tab), P(out), 2, 8, 8, 1) == 0
    torch.cuda.synchronize()
    n = 2 * 4 * 4 * 32
    assert bool((out[:n] == 0).all()) and bool((out[n:] == CANARY).all())
    out.fill_(CANARY)
    assert bwd(P(big), None, P(tab), P(big), P(out[1:]), 1, 2, 8, 8, 0) == 0
    torch.cuda.synchronize()
    n = 2 * 3 * 8 * 8
    assert float(out[0]) == CANARY and bool((out[1:1 + n] == 0).all()) and bool((out[1 + n:] == CANARY).all())


def test_first_conv_beyond_2_31_elements():
    """B = 5351 images at 224 x 224, bf16 streams: y, g and the mask source hold 2.148e9 elements, so the whole last image
    lies beyond element 2^31 (and 2^32 bytes).  The first and the last image equal the same images run alone, bit for bit,
    forward and gradient; operands of the clamp set, whose first image is also compared with the restatement."""
    _need(20)
    B, H, W = 5351, 224, 224
    OH, OW = fref.out_grid(H, W)
    assert B * OH * OW * 32 > 2 ** 31 and (B - 1) * OH * OW * 32 > 2 ** 31
    op = fref.operands("big", "clamp", 1, H, W, BF16)
    wf, wb, scale, shift = _dev(fref.pack_fwd(op.w)), _dev(fref.pack_bwd(op.w)), _dev(op.scale), _dev(op.shift)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)

    def fill(t, lo, hi):
        step = 256
        for b0 in range(0, t.shape[0], step):
            part = t[b0:b0 + step]
            part.copy_(torch.randint(lo, hi + 1, part.shape, generator=gen, device=DEV, dtype=torch.int8))
        return t

    x = fill(torch.empty((B, 3, H, W), dtype=BF16, device=DEV), -2, 2)
    x[0].copy_(op.x[0])
    y = _run_fwd(x, wf, op.mean, op.inv_std, scale, shift, 1)
    ref = fref.first_fwd(Arith(), op.x, op.w, op.mean, op.inv_std, op.scale, op.shift, 1)
    fref.assert_premise("big/fwd", ref)
    fref.compare_exact("big/fwd/0", y[:1], ref)
    for b in (0, B - 1):
        alone = _run_fwd(x[b:b + 1].contiguous(), wf, op.mean, op.inv_std, scale, shift, 1)
        assert _same_bits(y[b:b + 1], alone), b
    g = fill(torch.empty((B, OH, OW, 32), dtype=BF16, device=DEV), -3, 3)
    gx = _run_bwd(g, y, scale, wb, op.inv_std, H, W, 1, BF16)
    del x
    for b in (0, B - 1):
        alone = _run_bwd(g[b:b + 1].contiguous(), y[b:b + 1].contiguous(), scale, wb, op.inv_std, H, W, 1, BF16)
        assert _same_bits(gx[b:b + 1], alone) and bool((alone != 0).any()), b
    refb = fref.first_bwd(Arith(), g[:1].cpu(), y[:1].cpu(), op.scale, op.w, op.inv_std, H, W, 1, BF16)
    fref.assert_premise("big/bwd", refb)
    fref.compare_exact("big/bwd/0", gx[:1], refb)


AUTOGRAD_ROWS = [(2, 14, 14), (3, 7, 5), (2, 33, 35)]


@pytest.mark.parametrize("b,h,w", AUTOGRAD_ROWS)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_autograd_function_equals_the_c_abi_bitwise(b, h, w, dtype):
    """ops.first_conv3x3 on the attack's NCHW tensor: no copies in or out, the very bits of the C-ABI calls, the output in
    channels_last storage, the gradient in x's dtype and layout."""
    o = ops()
    op = fref.operands("autograd/%s" % ((b, h, w),), "gaussian", b, h, w, dtype)
    want_y = _fwd(op, 1)
    want_gx = _bwd(op, want_y, h, w, 1, dtype)
    wf, wb = o.pack_first3x3_weights(_dev(op.w))
    assert torch.equal(wf.reshape(32, 3, 4, 4), _dev(fref.pack_fwd(op.w))) and torch.equal(wb.reshape(3, 9, 32), _dev(fref.pack_bwd(op.w)))
    args = (wf, wb, _dev(op.scale), _dev(op.shift), op.mean, op.inv_std)
    x = _dev(op.x).requires_grad_(True)
    y = o.first_conv3x3(x, *args)
    oh, ow = fref.out_grid(h, w)
    assert y.shape == (b, 32, oh, ow) and y.dtype == BF16 and y.permute(0, 2, 3, 1).is_contiguous()
    assert _same_bits(y.detach().permute(0, 2, 3, 1), want_y)
    (gx,) = torch.autograd.grad(y, x, _dev(op.g).permute(0, 3, 1, 2))
    assert gx.shape == x.shape and gx.dtype == dtype and gx.is_contiguous()
    assert _same_bits(gx, want_gx)
    empty = o.first_conv3x3(x[:0].detach().requires_grad_(True), *args)           # B = 0 launches nothing
    assert empty.shape == (0, 32, oh, ow)
    with pytest.raises(ValueError):
        o.first_conv3x3(x.double(), *args)
    with pytest.raises(ValueError):
        o.first_conv3x3(x[:, :2], *args)
    with pytest.raises(ValueError):
        o.first_conv3x3(x, wf, wb, args[2].double(), args[3], op.mean, op.inv_std)
    with pytest.raises(ValueError):
        o.first_conv3x3(x, wf.float(), wb, args[2], args[3], op.mean, op.inv_std)


def test_first_conv_in_a_captured_graph():
    """Forward + input gradient captured in a graph on a single stream and replayed (on fresh inputs copied into the
    captured buffers) equals the eager result bit for bit: the calls launch on the capturing stream and neither synchronise
    nor allocate outside the allocator."""
    o = ops()
    b, h, w = 4, 33, 35
    op = fref.operands("graph", "gaussian", b, h, w, BF16)
    op2 = fref.operands("graph/2", "gaussian", b, h, w, BF16)
    wf, wb = o.pack_first3x3_weights(_dev(op.w))
    args = (wf, wb, _dev(op.scale), _dev(op.shift), op.mean, op.inv_std)
    nchw = lambda g: _dev(g).permute(0, 3, 1, 2)

    def run(x, g):
        y = o.first_conv3x3(x, *args)
        (gx,) = torch.autograd.grad(y, x, g)
        return y, gx

    eager = [tuple(t.detach().clone() for t in run(_dev(q.x).requires_grad_(True), nchw(q.g))) for q in (op, op2)]
    xs = _dev(op.x).clone().requires_grad_(True)
    gs = nchw(op.g).clone(memory_format=torch.preserve_format)
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
            xs.copy_(_dev(q.x))
            gs.copy_(nchw(q.g))
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(ys.detach().permute(0, 2, 3, 1), want_y.permute(0, 2, 3, 1))
        assert _same_bits(gxs, want_gx)


# ------------------------------------------------------------------------------------------------------------- network
def randomised_checkpoint(path, images=None, seed=5, num_classes=1000):
    """The recipe of tests/test_gpu_depthwise.py and tests/test_gpu_pointwise8.py, restated: a seeded MobileNetV2
    state_dict with randomised BatchNorm statistics and affine maps, so that every term of the epilogue tables is exercised.
    images None: statistics drawn around the initial 0 / 1 (mean 0.2 N(0,1), var in [0.6, 1.4], gamma in [0.7, 1.3], beta
      0.2 N(0,1)): the network of the precision comparisons.
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
    assert g.shape == x.shape and g.dtype == x.dtype
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


def test_mobilenet_on_own_first_conv_kernels(tmp_path, monkeypatch):
    """`own_first_conv=True` on 8 structured images at 224 x 224, a checkpoint with randomised BatchNorm statistics: the
    rewritten layer against the restatement applied to its actual input (gaussian bound, ratio printed), the library calls
    that are left (all three switches: none; this switch alone: the 17 grouped and 34 dense convolutions and their 51
    BatchNorms), the logits against the fp32 network within the bf16 depth bound of 53 layers, and the input gradient no
    further from the fp32 network's than 1.5 x the distance of the plain bf16 network (the parent path), for bf16 and fp32
    inputs."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import zoo
    images, _ = structured_images(8, classes=4, seed=3, size=224)
    path = randomised_checkpoint(os.path.join(str(tmp_path), "mobilenet_random_bn.pt"))
    kw = dict(num_classes=1000, seed=5, weights=path, device=DEV)
    ref = zoo.build_classifier("mobilenet", **kw)
    kw.update(dtype=BF16, channels_last=True)
    off = zoo.build_classifier("mobilenet", **kw)
    fc = zoo.build_classifier("mobilenet", own_first_conv=True, **kw)
    all3 = zoo.build_classifier("mobilenet", own_first_conv=True, own_pointwise=True, own_depthwise=True, **kw)
    x = images.to(DEV)
    seen = []

    def restate(mod, args, out):
        xin = args[0]
        assert xin.dtype == BF16 and xin.is_contiguous() and out.is_contiguous(memory_format=torch.channels_last)
        o = fref.first_fwd(Arith(), xin.detach(), mod[0].weight.detach(), mod.mean, mod.inv_std, mod.scale, mod.shift, 1)
        seen.append(fref.gaussian_ratio(out.detach().permute(0, 2, 3, 1), o))

    first = all3[0].features[0]
    assert isinstance(first, zoo._OwnFirstConv)
    handle = first.register_forward_hook(restate)
    calls = _Calls(monkeypatch)
    l2, g2 = _forward_and_gradient(all3, x.bfloat16())
    n_all3 = calls.take()
    handle.remove()
    l1, g1 = _forward_and_gradient(fc, x.bfloat16())
    n_fc = calls.take()
    l0, g0 = _forward_and_gradient(off, x.bfloat16())
    n_off = calls.take()
    monkeypatch.undo()
    print("library calls (grouped conv, dense conv, BatchNorm): off %s, own_first_conv %s, all three switches %s" % (n_off, n_fc, n_all3))
    assert n_off == (17, 35, 52) and n_all3 == (0, 0, 0) and n_fc == (17, 34, 51)
    assert len(seen) == 1
    print("first layer 3 -> 32 at 224 x 224 on its real input: max |err| / bound %.3f" % seen[0])
    assert seen[0] <= 1.0, seen
    l3, g3 = _forward_and_gradient(all3, x)                              # an fp32 stream into the bf16 network
    lr, gr = _forward_and_gradient(ref, x)
    rms = float(lr.square().mean().sqrt())
    bound = _bf16_depth_bound(53) * rms
    rel = lambda g: float((g - gr).norm() / gr.norm())
    e0, e1, e2, e3 = (float((l - lr).abs().mean()) for l in (l0, l1, l2, l3))
    r0, r1, r2, r3 = rel(g0), rel(g1), rel(g2), rel(g3)
    print("logit error vs fp32: off %.5f own_first_conv %.5f all three %.5f all three (fp32 x) %.5f, rms %.4f, bound %.5f; "
          "input gradient relative error vs fp32: off %.4f own_first_conv %.4f all three %.4f all three (fp32 x) %.4f"
          % (e0, e1, e2, e3, rms, bound, r0, r1, r2, r3))
    assert float(gr.abs().max()) > 0
    for l, g in ((l1, g1), (l2, g2), (l3, g3)):
        assert torch.isfinite(l).all() and torch.isfinite(g).all() and g.shape == x.shape and float(g.abs().max()) > 0
    assert max(e1, e2, e3) <= bound, (e0, e1, e2, e3, rms)
    assert max(r1, r2, r3) <= 1.5 * r0, (r0, r1, r2, r3)


def test_first_conv_is_bitwise_across_processes():
    """Two fresh child processes, one after the other (the second only if the first exited 0), each under `timeout`:
    byte-identical y and gx for three rows."""
    child = os.path.join(ROOT, "tests", "first_conv_child.py")
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
    with all three switches on.  All values finite, at least one image fooled; the count and the loss are printed."""
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
                                 own_depthwise=True, own_pointwise=True, own_first_conv=True)
    learner = engine.DictionaryLearner(d0.clone().to(DEV), v0.clone().to(DEV), eps, 0.01, "logits", False, 50.0)
    last = None
    for _ in range(20):
        ls, fl = learner.step(model, x, index)
        last = (float(ls), int(fl))
    assert torch.isfinite(learner.d).all() and torch.isfinite(learner.v).all() and last[0] == last[0]
    print("fooled after 20 steps of 32 images, all three switches on: %d (loss %.4f)" % (last[1], last[0]))
    assert last[1] >= 1, last
