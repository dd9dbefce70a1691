"""GPU: the VGG kernels (csrc/adil_conv3x3.hip, csrc/adil_bias_relu_pool2.hip) through the C ABI — adil_conv3x3_wide against the fp64 restatement
of tests/classifier_reference.py (bit for bit on the exact leg, under the derived elementwise bound on the gaussian leg),
adil_bias_relu_pool2_fwd / _bwd against torch's own fp32 chain and autograd on the CPU (bit for bit) — their autograd
wrappers, and the VGG11 that runs seven of its eight convolutions and all its ReLUs and pools on them (`own_vgg_conv`)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import vgg_conv_reference as vref
from classifier_reference import BF16, CANARY

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


def _dev(t):
    return t.to(DEV).contiguous()


def _conv(src, wp, B, H, W, R, O, entry="adil_conv3x3_wide"):
    """Device tensors in; the output [B H W][O] with canary rows behind it checked."""
    o, lib = ops(), _lib()
    M = B * H * W
    out = torch.full((M + PAD, O), CANARY, dtype=BF16, device=DEV)
    assert getattr(lib, entry)(o._ptr(src), o._ptr(wp), o._ptr(out), B, H, W, R, O, o._stream()) == 0
    torch.cuda.synchronize()
    assert bool((out[M:] == CANARY).all()), entry + " wrote past the end of its output"
    return out[:M]


def _fwd(x, wp, row):
    B, H, W, C, N = row
    return _conv(x, wp, B, H, W, C, N)


def _bwd(g, wp_bwd, row):
    B, H, W, C, N = row
    return _conv(g, wp_bwd, B, H, W, N, C)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("row", vref.ROWS, ids=str)
def test_wide_conv_against_the_fp64_restatement(row):
    """Forward and input gradient of one row: the exact leg bit for bit, the gaussian leg under the derived bound (ratio
    printed), canary rows behind the outputs intact, a second call identical in bits.  Rows and operands are those of
    tests/test_vgg_conv_cpu.py, where the emulation passes them and every premise is asserted on the reference alone."""
    name = vref.row_name(*row)
    r = vref.reference_row(row, "exact")
    x, g, wp, wp_bwd = _dev(r.ops.x), _dev(r.ops.g), _dev(r.wp), _dev(r.wp_bwd)
    y, gx = _fwd(x, wp, row), _bwd(g, wp_bwd, row)
    vref.compare_exact(name + "/exact/fwd", y.cpu(), r.fwd)
    vref.compare_exact(name + "/exact/bwd", gx.cpu(), r.bwd)
    r = vref.reference_row(row, "gaussian")
    x, g, wp, wp_bwd = _dev(r.ops.x), _dev(r.ops.g), _dev(r.wp), _dev(r.wp_bwd)
    y, gx = _fwd(x, wp, row), _bwd(g, wp_bwd, row)
    rf, rb = vref.gaussian_ratio(y.cpu(), r.fwd), vref.gaussian_ratio(gx.cpu(), r.bwd)
    print(name, "gaussian max |err| / bound: fwd %.3f bwd %.3f" % (rf, rb))
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)
    assert _same(_fwd(x, wp, row), y) and _same(_bwd(g, wp_bwd, row), gx)


@pytest.mark.parametrize("row", [(3, 6, 10, 64, 64), (1, 9, 15, 512, 64), (1, 7, 15, 64, 128), (2, 5, 9, 192, 128)], ids=str)
def test_wide_conv_gives_the_bits_of_adil_conv3x3_where_both_cover(row):
    """W <= 63: the linear-tile kernel and the 2-D-tile kernel run the same MFMAs per accumulator in the same order (one
    kernel body, csrc/adil_conv3x3.hip).  The rows reach <64, 4> with one and with eight channel chunks and <128, 2> with
    one and with three (the halo reload and the register rotation at a chunk boundary)."""
    r = vref.reference_row(row, "gaussian")
    B, H, W, C, N = row
    x, g, wp, wp_bwd = _dev(r.ops.x), _dev(r.ops.g), _dev(r.wp), _dev(r.wp_bwd)
    assert _same(_fwd(x, wp, row), _conv(x, wp, B, H, W, C, N, "adil_conv3x3"))
    assert _same(_bwd(g, wp_bwd, row), _conv(g, wp_bwd, B, H, W, N, C, "adil_conv3x3"))


def _in_nan(t):
    """The same values as a view into a larger buffer of NaN: 64 NaN directly in front of and behind the operand."""
    t = t.to(DEV).contiguous()
    buf = torch.full((t.numel() + 128,), float("nan"), dtype=t.dtype, device=DEV)
    buf[64:64 + t.numel()] = t.reshape(-1)
    v = buf[64:64 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 0 and bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all())
    return v


@pytest.mark.parametrize("row", vref.NAN_ROWS, ids=str)
def test_wide_conv_reads_nothing_outside_its_operands(row):
    """x, wp, g and wp_bwd surrounded by NaN: a halo pixel in front of the first or behind the last image is not read from
    outside the operand.  The results hold no NaN and equal the plain call (and the restatement) bit for bit."""
    name = vref.row_name(*row)
    r = vref.reference_row(row, "exact")
    plain_y, plain_gx = _fwd(_dev(r.ops.x), _dev(r.wp), row), _bwd(_dev(r.ops.g), _dev(r.wp_bwd), row)
    got_y, got_gx = _fwd(_in_nan(r.ops.x), _in_nan(r.wp), row), _bwd(_in_nan(r.ops.g), _in_nan(r.wp_bwd), row)
    assert bool(torch.isfinite(got_y).all()) and bool(torch.isfinite(got_gx).all())
    assert _same(got_y, plain_y) and _same(got_gx, plain_gx)
    vref.compare_exact(name + "/fwd", got_y.cpu(), r.fwd)
    vref.compare_exact(name + "/bwd", got_gx.cpu(), r.bwd)


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("row", vref.NAN_ROWS, ids=str)
def test_wide_conv_keeps_a_poisoned_image_to_itself(row, poison):
    """Image 1 of x (of g for the gradient) filled with NaN, and with +Inf: a halo pixel of its neighbours that leaves
    their image is a zero by selection, never a value of image 1 times zero — their outputs equal the clean call bit for
    bit and are finite."""
    B, H, W, C, N = row
    r = vref.reference_row(row, "exact")
    for run, src, wp, O in ((_fwd, r.ops.x, r.wp, N), (_bwd, r.ops.g, r.wp_bwd, C)):
        clean = run(_dev(src), _dev(wp), row).reshape(B, H * W, O)
        bad = _dev(src).clone()
        bad[1] = poison
        got = run(bad, _dev(wp), row).reshape(B, H * W, O)
        for img in sorted({0, B - 1} - {1}):
            assert bool(torch.isfinite(got[img]).all())
            assert _same(got[img], clean[img])
        assert not bool(torch.isfinite(got[1]).all())                 # the poison was really there


def test_refusals_on_the_device_leave_outputs_untouched():
    """The refusals of tests/test_vgg_conv_cpu.py on the device: ADIL_EINVAL, canary outputs intact after a synchronise;
    the accepted forms write their outputs alone."""
    o, lib = ops(), _lib()
    big = torch.zeros(1 << 20, dtype=BF16, device=DEV)
    bias = torch.zeros(64, dtype=torch.float32, device=DEV)
    out = torch.full((1 << 20,), CANARY, dtype=BF16, device=DEV)
    idx = torch.full((1 << 20,), 77, dtype=torch.uint8, device=DEV)
    P, S = o._ptr, o._stream
    f = lib.adil_conv3x3_wide
    for dims in vref.REFUSED_DIMS:
        assert f(P(big), P(big), P(out), *dims, S()) == EINVAL, dims
    good = [P(big), P(big), P(out)]
    for i in range(3):
        a = list(good)
        a[i] = None
        assert f(*a, 2, 4, 4, 64, 64, S()) == EINVAL, i
        a[i] = P(out[4:]) if i == 2 else P(big[4:])                # 8 bytes past a 16-byte boundary
        assert f(*a, 2, 4, 4, 64, 64, S()) == EINVAL, i
    assert f(*good, 2 ** 20, 2 ** 11, 1, 64, 64, S()) == EINVAL
    fwd, bwd = lib.adil_bias_relu_pool2_fwd, lib.adil_bias_relu_pool2_bwd
    for dims in vref.POOL_REFUSED_DIMS:
        assert fwd(P(big), P(bias), P(out), P(idx), *dims, S()) == EINVAL, dims
        assert bwd(P(big), P(idx), P(out), *dims, S()) == EINVAL, dims
    assert fwd(P(big), P(bias[1:]), P(out), P(idx), 2, 4, 4, 8, S()) == EINVAL
    assert fwd(P(big), P(bias), P(out[4:]), P(idx), 2, 4, 4, 8, S()) == EINVAL
    assert fwd(P(big), P(bias), P(out), P(idx[4:]), 2, 4, 4, 8, S()) == EINVAL
    assert fwd(P(big), P(bias), None, P(idx), 2, 4, 4, 8, S()) == EINVAL
    assert bwd(P(big), P(idx[4:]), P(out), 2, 4, 4, 8, S()) == EINVAL
    assert bwd(P(big), P(idx), P(out[4:]), 2, 4, 4, 8, S()) == EINVAL
    assert bwd(P(big), None, P(out), 2, 4, 4, 8, S()) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and bool((idx == 77).all())
    assert f(*good, 2, 4, 4, 64, 64, S()) == 0                         # the accepted form writes y alone
    torch.cuda.synchronize()
    assert bool((out[:2 * 4 * 4 * 64] == 0).all()) and bool((out[2 * 4 * 4 * 64:] == CANARY).all())


@pytest.mark.parametrize("row,bias", [(row, b) for row in vref.POOL_ROWS for b in (True, False)], ids=str)
@pytest.mark.parametrize("leg", ["tie", "gaussian"])
def test_pool_pair_equals_torch_bitwise(row, bias, leg):
    """y, idx and gx of one row against the restatement (which tests/test_vgg_conv_cpu.py holds to torch's fp32 chain and
    autograd) and against torch's results themselves, bit for bit, zeros' signs included; canaries behind y, idx and gx
    intact; a second call identical in bits."""
    o, lib = ops(), _lib()
    B, H, W, C = row
    r = vref.pool_reference(row, bias, leg)
    want = vref.pool_restate(r.ops)
    n_out, n_in = B * (H // 2) * (W // 2) * C, B * H * W * C
    x, g = _dev(r.ops.x), _dev(r.ops.g)
    b = None if r.ops.bias is None else _dev(r.ops.bias)

    def run():
        y = torch.full((n_out + PAD * C,), CANARY, dtype=BF16, device=DEV)
        idx = torch.full((n_out + PAD * C,), 77, dtype=torch.uint8, device=DEV)
        gx = torch.full((n_in + PAD * C,), CANARY, dtype=BF16, device=DEV)
        assert lib.adil_bias_relu_pool2_fwd(o._ptr(x), o._ptr(b), o._ptr(y), o._ptr(idx), B, H, W, C, o._stream()) == 0
        assert lib.adil_bias_relu_pool2_bwd(o._ptr(g), o._ptr(idx), o._ptr(gx), B, H, W, C, o._stream()) == 0
        torch.cuda.synchronize()
        assert bool((y[n_out:] == CANARY).all()) and bool((idx[n_out:] == 77).all()) and bool((gx[n_in:] == CANARY).all())
        return y[:n_out].cpu().view(want.y.shape), idx[:n_out].cpu().view(want.idx.shape), gx[:n_in].cpu().view(want.gx.shape)

    y, idx, gx = run()
    assert vref.same_bits(y, want.y) and vref.same_bits(idx, want.idx) and vref.same_bits(gx, want.gx)
    assert vref.same_bits(y, r.y) and vref.same_bits(gx, r.gx)
    y2, idx2, gx2 = run()
    assert vref.same_bits(y, y2) and vref.same_bits(idx, idx2) and vref.same_bits(gx, gx2)


def _nchw(t):
    return t.to(DEV).permute(0, 3, 1, 2)


@pytest.mark.parametrize("row", [(2, 5, 70, 64, 128), (1, 17, 65, 128, 64)], ids=str)
def test_conv_function_equals_the_c_abi_bitwise(row):
    """ops.conv3x3_wide on NCHW-shaped channels_last tensors with the weights of ops.pack_conv3x3_weights: the very bits
    of the C-ABI calls, channels_last outputs, no copy of x; ValueError on a wrong dtype, shape, layout or device; an empty
    batch gives empty tensors."""
    o = ops()
    B, H, W, C, N = row
    r = vref.reference_row(row, "gaussian")
    wf, wb = (t.to(DEV) for t in o.pack_conv3x3_weights(r.ops.w))
    assert torch.equal(wf.cpu().reshape(N, 9, C), r.wp)
    assert torch.equal(wb.cpu().reshape(C, 9, N), vref.pack_taps_flipped(r.ops.w))
    want_y, want_gx = _fwd(_dev(r.ops.x), wf, row), _bwd(_dev(r.ops.g), wb, row)
    x = _nchw(r.ops.x).requires_grad_(True)
    y = o.conv3x3_wide(x, wf, wb)
    assert y.shape == (B, N, H, W) and y.dtype == BF16 and y.permute(0, 2, 3, 1).is_contiguous()
    assert _same(y.detach().permute(0, 2, 3, 1).reshape(-1, N), want_y)
    (gx,) = torch.autograd.grad(y, (x,), _nchw(r.ops.g))
    assert gx.shape == x.shape and gx.dtype == BF16 and gx.permute(0, 2, 3, 1).is_contiguous()
    assert _same(gx.permute(0, 2, 3, 1).reshape(-1, C), want_gx)
    assert o._nhwc(x).data_ptr() == x.data_ptr()                                             # the kernel reads x in place
    assert o.conv3x3_wide_covers(x, C, N) and not o.conv3x3_wide_covers(x, C - 32, N)
    xd = x.detach()
    for bad in (lambda: o.conv3x3_wide(xd.float(), wf, wb),                                  # dtype
                lambda: o.conv3x3_wide(xd[:, :C - 32], wf, wb),                              # channel count
                lambda: o.conv3x3_wide(xd[0], wf, wb),                                       # 3-d
                lambda: o.conv3x3_wide(xd.contiguous(), wf, wb),                             # NCHW storage
                lambda: o.conv3x3_wide(xd.cpu(), wf, wb),                                    # device
                lambda: o.conv3x3_wide(xd, wf.cpu(), wb),
                lambda: o.conv3x3_wide(xd, wf.float(), wb),
                lambda: o.conv3x3_wide(xd, wf, wb[:, :-9]),
                lambda: o.conv3x3_wide(xd, wf.reshape(N, 9, C), wb),
                lambda: o.conv3x3_wide(xd, wf, wb.t())):
        with pytest.raises(ValueError):
            bad()
    x0 = xd[:0].requires_grad_(True)
    y0 = o.conv3x3_wide(x0, wf, wb)
    assert y0.shape == (0, N, H, W) and y0.dtype == BF16
    (g0,) = torch.autograd.grad(y0, (x0,), torch.zeros_like(y0))
    assert g0.shape == (0, C, H, W)


@pytest.mark.parametrize("row,bias", [((2, 6, 10, 16), True), ((3, 8, 8, 72), False)], ids=str)
def test_pool_function_equals_torch_bitwise(row, bias):
    """ops.bias_relu_pool2 on NCHW-shaped channels_last tensors through autograd: torch's bits, channels_last outputs, only
    the byte index saved, no gradient for the bias; ValueError on uncovered input; an empty batch gives empty tensors."""
    o = ops()
    B, H, W, C = row
    r = vref.pool_reference(row, bias, "tie")
    b = None if r.ops.bias is None else _dev(r.ops.bias).requires_grad_(True)
    x = _nchw(r.ops.x).requires_grad_(True)
    y = o.bias_relu_pool2(x, b)
    assert y.shape == (B, C, H // 2, W // 2) and y.dtype == BF16 and y.permute(0, 2, 3, 1).is_contiguous()
    assert vref.same_bits(y.detach().permute(0, 2, 3, 1).cpu(), r.y)
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].dtype == torch.uint8 and saved[0].shape == (B, H // 2, W // 2, C)
    grads = torch.autograd.grad(y, (x,) if b is None else (x, b), _nchw(r.ops.g), allow_unused=True)
    assert grads[0].shape == x.shape and grads[0].dtype == BF16 and grads[0].permute(0, 2, 3, 1).is_contiguous()
    assert vref.same_bits(grads[0].permute(0, 2, 3, 1).cpu(), r.gx)
    assert b is None or grads[1] is None
    xd, bd = x.detach(), None if b is None else b.detach()
    assert o.bias_relu_pool2_covers(xd) and not o.bias_relu_pool2_covers(xd[:, :, :-1])
    bads = [lambda: o.bias_relu_pool2(xd.float(), bd),                                       # dtype
            lambda: o.bias_relu_pool2(xd[:, :, :-1], bd),                                    # odd H
            lambda: o.bias_relu_pool2(xd[:, :, :, :-1], bd),                                 # odd W
            lambda: o.bias_relu_pool2(xd[:, :C - 4], None),                                  # C % 8
            lambda: o.bias_relu_pool2(xd[0], bd),                                            # 3-d
            lambda: o.bias_relu_pool2(xd.contiguous(), bd),                                  # NCHW storage
            lambda: o.bias_relu_pool2(xd.cpu(), None)]                                       # device
    if bd is not None:
        bads += [lambda: o.bias_relu_pool2(xd, bd[:-8]), lambda: o.bias_relu_pool2(xd, bd.bfloat16()),
                 lambda: o.bias_relu_pool2(xd, bd.cpu())]
    for bad in bads:
        with pytest.raises(ValueError):
            bad()
    x0 = xd[:0].requires_grad_(True)
    y0 = o.bias_relu_pool2(x0, bd)
    assert y0.shape == (0, C, H // 2, W // 2) and y0.dtype == BF16
    (g0,) = torch.autograd.grad(y0, (x0,), torch.zeros_like(y0))
    assert g0.shape == (0, C, H, W)


def test_one_group_in_a_captured_graph():
    """One group (conv3x3_wide -> bias_relu_pool2, forward + input gradient, 2 x 8 x 80, 64 -> 64) captured in a graph and
    replayed on two input sets equals the eager result bit for bit: the calls launch on the capturing stream and neither
    synchronise nor allocate outside the allocator."""
    o = ops()
    B, H, W, C, N = 2, 8, 80, 64, 64
    sets = [vref.operands("graph/%d" % i, "gaussian", B, H, W, C, N) for i in range(2)]
    wf, wb = (t.to(DEV) for t in o.pack_conv3x3_weights(sets[0].w))
    bias = (0.5 * torch.randn(N, generator=torch.Generator().manual_seed(3))).to(DEV)

    def run(x, g):
        y = o.bias_relu_pool2(o.conv3x3_wide(x, wf, wb), bias)
        (gx,) = torch.autograd.grad(y, x, g)
        return y, gx

    pooled = lambda q: _nchw(q.g)[:, :, ::2, ::2].contiguous(memory_format=torch.channels_last)
    eager = [tuple(t.detach().clone() for t in run(_nchw(q.x).requires_grad_(True), pooled(q))) for q in sets]
    assert float(eager[0][0].abs().max()) > 0 and float(eager[0][1].abs().max()) > 0
    xs = _nchw(sets[0].x).clone(memory_format=torch.preserve_format).requires_grad_(True)
    gs = pooled(sets[0]).clone(memory_format=torch.preserve_format)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(xs, gs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys, gxs = run(xs, gs)
    for q, (want_y, want_gx) in zip(sets, eager):
        with torch.no_grad():
            xs.copy_(_nchw(q.x))
            gs.copy_(pooled(q))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(ys.detach().permute(0, 2, 3, 1), want_y.permute(0, 2, 3, 1))
        assert _same(gxs.permute(0, 2, 3, 1), want_gx.permute(0, 2, 3, 1))


def test_vgg_kernels_are_bitwise_across_processes():
    """Two fresh child processes, one after the other (the second only if the first exited 0), each under `timeout`:
    byte-identical hashes of three wide rows and two pool rows, outputs and input gradients."""
    child = os.path.join(ROOT, "tests", "vgg_conv_child.py")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
    outs = []
    for _ in range(2):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, child], env=env, capture_output=True, text=True,
                           timeout=270, cwd=ROOT)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("hash ")]
        assert len(lines) == 10, r.stdout[-2000:]              # three wide rows and two pool rows, output and gradient
        outs.append(lines)
    for a, b in zip(*outs):
        assert a == b, (a, b)


# ------------------------------------------------------------------------------------------------------------- network
def vgg_checkpoint(path, seed=5, num_classes=1000):
    """A seeded VGG11 state_dict with kaiming fan-out convolution weights (what torchvision initialises VGG with) and
    biases N(0, 0.1), so that the bias path is under test."""
    from dl_attack_on_imagenet_amd import zoo
    model = zoo.build_classifier("vgg11", num_classes=num_classes, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.Conv2d):
                std = (2.0 / (m.out_channels * 9)) ** 0.5
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * std)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
    torch.save(model[1].state_dict(), path)
    return path


def _forward_and_gradient(model, x):
    x = x.clone().requires_grad_(True)
    logits = model(x).float()
    (g,) = torch.autograd.grad(logits.square().sum(), x)
    return logits.detach(), g.detach().float()


@pytest.fixture(scope="module")
def networks(tmp_path_factory):
    """What the network cases share, built once and left unchanged: the checkpoint, the fp32 network, the plain bf16
    network and the switched one (16 classes: the 25088 x 4096 linear layer dominates the build as it is)."""
    from dl_attack_on_imagenet_amd import zoo
    path = vgg_checkpoint(os.path.join(str(tmp_path_factory.mktemp("vgg")), "vgg11_kaiming.pt"), num_classes=16)
    kw = dict(num_classes=16, seed=5, weights=path, device=DEV)
    fp32 = zoo.build_classifier("vgg11", **kw)
    kw.update(dtype=BF16, channels_last=True)
    return fp32, zoo.build_classifier("vgg11", **kw), zoo.build_classifier("vgg11", own_vgg_conv=True, **kw)


def _count(mp, obj, name, log, key=lambda a: None):
    real = getattr(obj, name)
    mp.setattr(obj, name, lambda *a, **k: (log.append((name, key(a))), real(*a, **k))[1])


def _network_case(networks, size):
    from structured import structured_images
    fp32, plain, own = networks
    images, _ = structured_images(2, classes=2, seed=3, size=size)
    x = images.to(DEV)
    lr, gr = _forward_and_gradient(fp32, x)
    l0, g0 = _forward_and_gradient(plain, x.bfloat16())
    l1, g1 = _forward_and_gradient(own, x.bfloat16())
    rel = lambda g: float((g - gr).norm() / gr.norm())
    e0, e1, r0, r1 = float((l0 - lr).abs().mean()), float((l1 - lr).abs().mean()), rel(g0), rel(g1)
    rms = float(lr.square().mean().sqrt())
    print("VGG11 at %d x %d: mean |logit error| vs fp32: plain bf16 %.5f, own_vgg_conv %.5f (rms logit %.4f; own / "
          "(2 * 2^-9 * sqrt(11) * rms) = %.3f); input gradient relative error vs fp32: plain %.4f own %.4f"
          % (size, size, e0, e1, rms, e1 / (2 * 2.0 ** -9 * 11 ** 0.5 * rms), r0, r1))
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all() and g1.shape == x.shape
    assert float(l1.abs().max()) > 0 and float(g1.abs().max()) > 0 and float(gr.abs().max()) > 0
    assert e1 <= 1.5 * e0, (e0, e1)
    assert r1 <= 1.5 * r0, (r0, r1)
    return own, x


def test_vgg11_on_own_kernels(networks, monkeypatch):
    """`own_vgg_conv=True` on 2 structured images at 128 x 128 (layer 2 then runs at W = 64 in the wide kernel, layers 3-8
    at 32, 32, 16, 16, 8, 8 in adil_conv3x3) and a checkpoint with kaiming fan-out weights and N(0, 0.1) biases: F.conv2d is
    reached once (the 3 -> 64 first convolution), F.max_pool2d never, F.relu twice (the classifier); the kernels are
    reached 1 + 6 + 5 + 3 times; against the fp32 network the mean |logit error| and the input gradient's relative error
    are at most 1.5 x the plain bf16 library network's own distance (which is not reproducible call to call); logits and
    gradient finite and non-zero.  The ratio to 2 * 2^-9 * sqrt(11) * rms logit is printed, not asserted."""
    o = ops()
    own, x = _network_case(networks, 128)
    log = []
    with monkeypatch.context() as mp:
        _count(mp, F, "conv2d", log, lambda a: tuple(a[1].shape))
        _count(mp, F, "max_pool2d", log)
        _count(mp, F, "relu", log)
        _count(mp, o, "conv3x3_wide", log, lambda a: a[0].shape[3])
        _count(mp, o, "conv3x3", log, lambda a: a[0].shape[3])
        _count(mp, o, "bias_relu_pool2", log, lambda a: a[0].shape[3])
        _count(mp, o, "affine_act", log, lambda a: a[0].shape[3])
        with torch.no_grad():
            own(x.bfloat16())
    calls = lambda n: [k for name, k in log if name == n]
    assert calls("conv2d") == [(64, 3, 3, 3)], log
    assert calls("max_pool2d") == [] and len(calls("relu")) == 2, log
    assert calls("conv3x3_wide") == [64] and calls("conv3x3") == [32, 32, 16, 16, 8, 8], log
    assert calls("bias_relu_pool2") == [128, 64, 32, 16, 8] and calls("affine_act") == [32, 16, 8], log


def test_vgg11_falls_back_group_by_group_on_odd_grids(networks, monkeypatch):
    """The same networks on 126 x 126 images: the grids are 126, 63, 31, 15, 7, so every pooled group behind the first
    meets an odd grid and keeps its original modules, while the first group and the unpooled ones stay on the kernels; the
    switched network still agrees with the fp32 one within the criterion of the 128 x 128 case."""
    o = ops()
    own, x = _network_case(networks, 126)
    log = []
    with monkeypatch.context() as mp:
        _count(mp, F, "max_pool2d", log)
        _count(mp, o, "bias_relu_pool2", log, lambda a: a[0].shape[3])
        _count(mp, o, "affine_act", log, lambda a: a[0].shape[3])
        with torch.no_grad():
            own(x.bfloat16())
    assert [k for n, k in log if n == "bias_relu_pool2"] == [126], log
    assert [k for n, k in log if n == "affine_act"] == [31, 15, 7], log
    assert len([1 for n, _ in log if n == "max_pool2d"]) == 4, log


def test_learner_steps_against_vgg11_reported(networks):
    """Reported leg, finite values only: 10 learner steps (bf16 streams, 8 structured images at 128 x 128, K = 10) against
    the switched VGG11; the loss and the number of fooled images are printed."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import engine
    model = networks[2]
    size, n, k, eps = 128, 8, 10, EPS_LEARNER
    images, _ = structured_images(n, classes=4, seed=7, size=size, noise=0.15)
    x = images.to(DEV).bfloat16().contiguous()
    gen = torch.Generator().manual_seed(0)
    d0 = -1 + 2 * torch.rand(3, size, size, k, generator=gen)
    v0 = ops().l1ball_project_(torch.rand(n, k, generator=gen).to(DEV), eps).cpu()
    index = torch.arange(n, device=DEV)
    learner = engine.DictionaryLearner(d0.clone().to(DEV), v0.clone().to(DEV), eps, 0.01, "logits", False, 50.0)
    last = None
    for _ in range(10):
        ls, fl = learner.step(model, x, index)
        last = (float(ls), int(fl))
    assert torch.isfinite(learner.d).all() and torch.isfinite(learner.v).all() and last[0] == last[0]
    print("fooled after 10 steps of %d images, own_vgg_conv on: %d (loss %.4f)" % (n, last[1], last[0]))
