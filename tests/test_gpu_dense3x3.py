"""GPU: the 32-channel 3x3 convolution kernels (adil_dense3x3_fwd / adil_dense3x3_bwd, csrc/adil_dense3x3.hip) through
the C ABI against the fp64 restatement of tests/classifier_reference.py — bit for bit on the exact leg, under the derived
elementwise bound on the gaussian leg — and the DenseNet-121 that runs its 58 growth convolutions on them
(`own_dense_conv=True`), alone and next to `own_dense_pointwise`."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import dense3x3_reference as dref
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


def _bf16_depth_bound(layers: int) -> float:
    """The bound of tests/test_gpu_stem.py, restated: mean |logit error| of a bf16-activation network against its fp32
    twin relative to the rms logit; `layers` roundings of relative size 2^-9 in series add in quadrature, times 2 for a
    relative gain above 1 in a random-weight network."""
    return 2.0 * 2.0 ** -9 * layers ** 0.5


def _dev(t):
    return t.to(DEV).contiguous()


def _run(entry, src, wp, B, H, W, C, N):
    """Device tensors in; the output [B H W][O] with canary rows behind it checked."""
    o, lib = ops(), _lib()
    M, O = B * H * W, wp.shape[0]
    out = torch.full((M + PAD, O), CANARY, dtype=BF16, device=DEV)
    assert getattr(lib, entry)(o._ptr(src), o._ptr(wp), o._ptr(out), B, H, W, C, N, o._stream()) == 0
    torch.cuda.synchronize()
    assert bool((out[M:] == CANARY).all()), entry + " wrote past the end of its output"
    return out[:M]


def _fwd(x, wp, row):
    return _run("adil_dense3x3_fwd", x, wp, *row)


def _bwd(g, wp_bwd, row):
    return _run("adil_dense3x3_bwd", g, wp_bwd, *row)


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("row", dref.ROWS, ids=str)
def test_dense3x3_against_the_fp64_restatement(row):
    """Forward and input gradient of one row: the exact leg bit for bit, the gaussian leg under the derived bound (ratio
    printed), canary rows behind the outputs intact, a second call identical in bits.  Rows and operands are those of
    tests/test_dense3x3_cpu.py, where the emulation passes them and every premise is asserted on the reference alone."""
    name = dref.row_name(*row)
    r = dref.reference_row(row, "exact")
    x, g, wp, wp_bwd = _dev(r.ops.x), _dev(r.ops.g), _dev(r.wp), _dev(r.wp_bwd)
    y, gx = _fwd(x, wp, row), _bwd(g, wp_bwd, row)
    geom = (dref.TILE, 32, (y.shape[0] + dref.TILE - 1) // dref.TILE, 1)
    dref.compare_exact(name + "/exact/fwd", y.cpu(), r.fwd, geom)
    dref.compare_exact(name + "/exact/bwd", gx.cpu(), r.bwd, geom)
    r = dref.reference_row(row, "gaussian")
    x, g, wp, wp_bwd = _dev(r.ops.x), _dev(r.ops.g), _dev(r.wp), _dev(r.wp_bwd)
    y, gx = _fwd(x, wp, row), _bwd(g, wp_bwd, row)
    rf, rb = dref.gaussian_ratio(y.cpu(), r.fwd), dref.gaussian_ratio(gx.cpu(), r.bwd)
    print(name, "gaussian max |err| / bound: fwd %.3f bwd %.3f" % (rf, rb))
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)
    assert _same(_fwd(x, wp, row), y) and _same(_bwd(g, wp_bwd, row), gx)


def _in_nan(t):
    """The same values as a view into a larger buffer of NaN: 64 NaN directly in front of and behind the operand."""
    t = t.to(DEV).contiguous()
    buf = torch.full((t.numel() + 128,), float("nan"), dtype=t.dtype, device=DEV)
    buf[64:64 + t.numel()] = t.reshape(-1)
    v = buf[64:64 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 0 and bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all())
    return v


@pytest.mark.parametrize("row", dref.NAN_ROWS, ids=str)
def test_dense3x3_reads_nothing_outside_its_operands(row):
    """x, wp, g and wp_bwd surrounded by NaN: the halo rows in front of the first and behind the last pixel are not read
    from outside the operand.  The results hold no NaN and equal the plain call (and the restatement) bit for bit."""
    name = dref.row_name(*row)
    r = dref.reference_row(row, "exact")
    plain_y, plain_gx = _fwd(_dev(r.ops.x), _dev(r.wp), row), _bwd(_dev(r.ops.g), _dev(r.wp_bwd), row)
    got_y, got_gx = _fwd(_in_nan(r.ops.x), _in_nan(r.wp), row), _bwd(_in_nan(r.ops.g), _in_nan(r.wp_bwd), row)
    assert not bool(torch.isnan(got_y).any()) and not bool(torch.isnan(got_gx).any())
    assert _same(got_y, plain_y) and _same(got_gx, plain_gx)
    dref.compare_exact(name + "/fwd", got_y.cpu(), r.fwd)
    dref.compare_exact(name + "/bwd", got_gx.cpu(), r.bwd)


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_dense3x3_masks_by_selection(poison):
    """Image 1 of x (of g for the gradient) filled with NaN, and with +Inf: a tap of images 0 and 2 that would read it in
    the linear pixel tiling is selected away, not multiplied by zero — their outputs equal the clean call bit for bit and
    are finite."""
    row = dref.MASK_ROW
    B, H, W, C, N = row
    r = dref.reference_row(row, "exact")
    for run, src, wp, O in ((_fwd, r.ops.x, r.wp, N), (_bwd, r.ops.g, r.wp_bwd, C)):
        clean = run(_dev(src), _dev(wp), row).reshape(B, H * W, O)
        bad = _dev(src).clone()
        bad[1] = poison
        got = run(bad, _dev(wp), row).reshape(B, H * W, O)
        for img in (0, 2):
            assert bool(torch.isfinite(got[img]).all())
            assert _same(got[img], clean[img])
        assert not bool(torch.isfinite(got[1]).all())                 # the poison was really there


def test_dense3x3_refuses_and_leaves_outputs_untouched():
    """The refusals of tests/test_dense3x3_cpu.py on the device: ADIL_EINVAL, canary outputs intact after a synchronise."""
    o, lib = ops(), _lib()
    big = torch.zeros(1 << 20, dtype=BF16, device=DEV)
    out = torch.full((1 << 20,), CANARY, dtype=BF16, device=DEV)
    P, S = o._ptr, o._stream
    for f in (lib.adil_dense3x3_fwd, lib.adil_dense3x3_bwd):
        for dims in dref.REFUSED_DIMS:
            assert f(P(big), P(big), P(out), *dims, S()) == EINVAL, dims
        good = [P(big), P(big), P(out)]
        for i in range(3):
            a = list(good)
            a[i] = None
            assert f(*a, 2, 4, 4, 32, 32, S()) == EINVAL, i
            a[i] = P(out[4:]) if i == 2 else P(big[4:])            # 8 bytes past a 16-byte boundary
            assert f(*a, 2, 4, 4, 32, 32, S()) == EINVAL, i
        assert f(*good, 2 ** 20, 2 ** 11, 1, 32, 32, S()) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    assert lib.adil_dense3x3_fwd(P(big), P(big), P(out), 2, 4, 4, 32, 32, S()) == 0       # the accepted form writes y alone
    torch.cuda.synchronize()
    assert bool((out[:2 * 4 * 4 * 32] == 0).all()) and bool((out[2 * 4 * 4 * 32:] == CANARY).all())


def _nchw(t):
    return t.to(DEV).permute(0, 3, 1, 2)


@pytest.mark.parametrize("row", [(1, 14, 14, 128, 32), (3, 22, 18, 160, 96)], ids=str)
def test_autograd_function_equals_the_c_abi_bitwise(row):
    """ops.dense3x3_conv on NCHW-shaped channels_last tensors with the weights of ops.pack_conv3x3_weights: the very bits
    of the C-ABI calls, channels_last outputs, no copy of x; ValueError on a wrong dtype, shape, layout or device; an empty
    batch gives empty tensors."""
    o = ops()
    B, H, W, C, N = row
    r = dref.reference_row(row, "gaussian")
    wf, wb = (t.to(DEV) for t in o.pack_conv3x3_weights(r.ops.w))
    assert torch.equal(wf.cpu().reshape(N, 9, C), r.wp)
    assert torch.equal(wb.cpu().reshape(C, 9, N), dref.pack_taps_flipped(r.ops.w))
    want_y, want_gx = _fwd(_dev(r.ops.x), wf, row), _bwd(_dev(r.ops.g), wb, row)
    x = _nchw(r.ops.x).requires_grad_(True)
    y = o.dense3x3_conv(x, wf, wb)
    assert y.shape == (B, N, H, W) and y.dtype == BF16 and y.permute(0, 2, 3, 1).is_contiguous()
    assert _same(y.detach().permute(0, 2, 3, 1).reshape(-1, N), want_y)
    (gx,) = torch.autograd.grad(y, (x,), _nchw(r.ops.g))
    assert gx.shape == x.shape and gx.dtype == BF16 and gx.permute(0, 2, 3, 1).is_contiguous()
    assert _same(gx.permute(0, 2, 3, 1).reshape(-1, C), want_gx)
    xd = x.detach()
    for bad in (lambda: o.dense3x3_conv(xd.float(), wf, wb),                                  # dtype
                lambda: o.dense3x3_conv(xd[:, :C - 32], wf, wb),                              # channel count
                lambda: o.dense3x3_conv(xd[0], wf, wb),                                       # 3-d
                lambda: o.dense3x3_conv(xd.contiguous(), wf, wb),                             # NCHW storage
                lambda: o.dense3x3_conv(xd.cpu(), wf, wb),                                    # device
                lambda: o.dense3x3_conv(xd, wf.cpu(), wb),
                lambda: o.dense3x3_conv(xd, wf.float(), wb),
                lambda: o.dense3x3_conv(xd, wf, wb[:, :-9]),
                lambda: o.dense3x3_conv(xd, wf.reshape(N, 9, C), wb),
                lambda: o.dense3x3_conv(xd, wf, wb.t()),
                lambda: o.dense3x3_conv(torch.cat([xd] * 5, 3)[..., :64], wf, wb)):           # W = 64
        with pytest.raises(ValueError):
            bad()
    x0 = xd[:0].requires_grad_(True)
    y0 = o.dense3x3_conv(x0, wf, wb)
    assert y0.shape == (0, N, H, W) and y0.dtype == BF16
    (g0,) = torch.autograd.grad(y0, (x0,), torch.zeros_like(y0))
    assert g0.shape == (0, C, H, W)


def test_dense3x3_in_a_captured_graph():
    """One layer's forward + input gradient (4 x 14 x 14, 128 -> 32) captured in a graph and replayed on two input sets
    equals the eager result bit for bit: the calls launch on the capturing stream and neither synchronise nor allocate
    outside the allocator."""
    o = ops()
    B, H, W, C, N = 4, 14, 14, 128, 32
    sets = [dref.operands("graph/%d" % i, "gaussian", B, H, W, C, N) for i in range(2)]
    wf, wb = (t.to(DEV) for t in o.pack_conv3x3_weights(sets[0].w))

    def run(x, g):
        y = o.dense3x3_conv(x, wf, wb)
        (gx,) = torch.autograd.grad(y, x, g)
        return y, gx

    eager = [tuple(t.detach().clone() for t in run(_nchw(q.x).requires_grad_(True), _nchw(q.g))) for q in sets]
    xs = _nchw(sets[0].x).clone(memory_format=torch.preserve_format).requires_grad_(True)
    gs = _nchw(sets[0].g).clone(memory_format=torch.preserve_format)
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
            gs.copy_(_nchw(q.g))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(ys.detach().permute(0, 2, 3, 1), want_y.permute(0, 2, 3, 1))
        assert _same(gxs.permute(0, 2, 3, 1), want_gx.permute(0, 2, 3, 1))


def test_dense3x3_is_bitwise_across_processes():
    """Two fresh child processes, one after the other (the second only if the first exited 0), each under `timeout`:
    byte-identical y and gx for three rows."""
    child = os.path.join(ROOT, "tests", "dense3x3_child.py")
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


# ------------------------------------------------------------------------------------------------------------- network
def randomised_checkpoint(path, images=None, seed=5, num_classes=1000):
    """The recipe of tests/test_gpu_dense1x1.randomised_checkpoint, restated: a seeded DenseNet-121 state_dict with
    randomised BatchNorm statistics and affine maps.
    images None: statistics drawn around the initial 0 / 1, gamma of BOTH signs, for the precision comparisons.
    images given: the statistics of those images (one training-mode pass) perturbed channel by channel, gamma of both
      signs: a network that stays alive through its 120 convolutions, for the learner leg."""
    from dl_attack_on_imagenet_amd import zoo
    model = zoo.build_classifier("densenet121", num_classes=num_classes, seed=seed)
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    gen = torch.Generator().manual_seed(seed + 1)
    r = lambda n: torch.randn(n, generator=gen)
    u = lambda n: torch.rand(n, generator=gen)
    sign = lambda n: (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()
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
                m.weight.copy_((0.7 + 0.6 * u(n)) * sign(n))
                m.bias.copy_(0.2 * r(n))
                m.running_mean.copy_(0.2 * r(n))
                m.running_var.copy_(0.6 + 0.8 * u(n))
            else:
                m.running_mean.mul_(1 + 0.2 * r(n)).add_(0.1 * m.running_var.sqrt() * r(n))
                m.running_var.mul_(0.6 + 0.8 * u(n))
                m.weight.copy_((0.7 + 0.6 * u(n)) * sign(n))
                m.bias.copy_(0.3 * r(n))
    torch.save(model[1].state_dict(), path)
    return path


def _forward_and_gradient(model, x):
    x = x.clone().requires_grad_(True)
    logits = model(x).float()
    (g,) = torch.autograd.grad(logits.square().sum(), x)
    return logits.detach(), g.detach().float()


@pytest.fixture(scope="module")
def plain_networks(tmp_path_factory):
    """What both network cases compare against, computed once and left unchanged: the images, the build arguments, the
    fp32 network's logits and input gradient and the plain bf16 network's."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import zoo
    images, _ = structured_images(4, classes=4, seed=3, size=64)
    path = randomised_checkpoint(os.path.join(str(tmp_path_factory.mktemp("dense3x3")), "densenet_random_bn.pt"))
    kw = dict(num_classes=1000, seed=5, weights=path, device=DEV)
    x = images.to(DEV)
    lr, gr = _forward_and_gradient(zoo.build_classifier("densenet121", **kw), x)
    kw.update(dtype=BF16, channels_last=True)
    l0, g0 = _forward_and_gradient(zoo.build_classifier("densenet121", **kw), x.bfloat16())
    return x, kw, (lr, gr), (l0, g0)


@pytest.mark.parametrize("both", [False, True], ids=["own_dense_conv", "both_switches"])
def test_densenet_on_own_dense_conv_kernels(plain_networks, monkeypatch, both):
    """`own_dense_conv=True`, alone and with `own_dense_pointwise`, on 4 structured images at 64 x 64 and a checkpoint with
    randomised BatchNorm statistics: each of the 58 rewritten convolutions against the restatement applied to its actual
    input (gaussian bound, ratio printed), the layers seen in network order, the logits against the fp32 network within
    the bf16 depth bound of 121 layers, the input gradient no further from the fp32 network's than 1.5 x the distance of
    the plain bf16 network.  With both switches F.conv2d is reached once per forward (the stem) and two fresh builds give
    bitwise equal logits and input gradients.
    Recorded on an MI355X: the 58 layers at 0.682-0.840 of their elementwise bound alone, 0.694-0.868 with both switches;
    mean |logit error| 0.00534 off / 0.00522 own_dense_conv / 0.00281 both, rms logit 0.6155, bound 0.02645;
    input-gradient relative error 0.1396 off / 0.1397 own_dense_conv / 0.1315 both (the "off" figures are library
    convolutions, which are not reproducible call to call)."""
    from dl_attack_on_imagenet_amd import zoo
    x, kw, (lr, gr), (l0, g0) = plain_networks
    size = x.shape[-1]
    rms = float(lr.square().mean().sqrt())
    bound = _bf16_depth_bound(121) * rms
    rel = lambda g: float((g - gr).norm() / gr.norm())
    e0, r0 = float((l0 - lr).abs().mean()), rel(g0)
    assert float(gr.abs().max()) > 0
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1)
    own = zoo.build_classifier("densenet121", own_dense_conv=True, own_dense_pointwise=both, **kw)
    seen = []

    def restate(mod, args, out):
        xin = args[0]
        assert xin.dtype == BF16 and xin.is_contiguous(memory_format=torch.channels_last)
        o = dref.conv3x3(Arith(), nhwc(xin), mod.weight.detach())["y"]
        seen.append((mod.in_channels, mod.out_channels, xin.shape[2], dref.gaussian_ratio(nhwc(out), o)))

    handles = [m.register_forward_hook(restate) for m in own.modules() if isinstance(m, zoo._OwnGrowthConv)]
    assert len(handles) == 58
    l1, g1 = _forward_and_gradient(own, x.bfloat16())
    for h in handles:
        h.remove()
    # the network's list at this size: every grid scales with the image (56, 28, 14, 7 at 224 -> 16, 8, 4, 2 at 64)
    assert [s[:3] for s in seen] == [(c, n, h * size // 224) for c, n, h in dref.DENSENET_GROWTH_LAYERS]
    worst = max(s[3] for s in seen)
    print("both switches" if both else "own_dense_conv alone", ": 58 layers, max |err| / bound %.3f .. %.3f"
          % (min(s[3] for s in seen), worst))
    assert worst <= 1.0, [s for s in seen if s[3] > 1.0]
    e1, r1 = float((l1 - lr).abs().mean()), rel(g1)
    print("logit error vs fp32: off %.5f own %.5f, rms %.4f, bound %.5f; input gradient relative error vs fp32: off %.4f "
          "own %.4f" % (e0, e1, rms, bound, r0, r1))
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all() and g1.shape == x.shape and float(g1.abs().max()) > 0
    assert e1 <= bound, (e0, e1, rms)
    assert r1 <= 1.5 * r0, (r0, r1)
    if both:
        calls, real = [], F.conv2d
        with monkeypatch.context() as mp:
            mp.setattr(F, "conv2d", lambda *a, **k: (calls.append(tuple(a[1].shape)), real(*a, **k))[1])
            with torch.no_grad():
                own(x.bfloat16())
        assert calls == [(64, 3, 7, 7)], calls                       # the stem alone
        again = zoo.build_classifier("densenet121", own_dense_conv=True, own_dense_pointwise=True, **kw)
        l2, g2 = _forward_and_gradient(again, x.bfloat16())
        assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_learner_steps_against_densenet_reported(tmp_path):
    """Reported leg, sanity bounds only: 20 learner steps (bf16 streams, 16 structured images at 64 x 64, K = 10) against
    DenseNet-121 with both DenseNet switches on and a head fitted by `fit_centroid_head` ON the switched network.  All
    values finite, at least one image fooled; the counts are printed.
    Recorded on an MI355X: the fitted head classifies 16 of 16 images, least margin 1.486; 6 images fooled after 20 steps,
    loss -14.4170."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import engine, zoo
    size, n, k, eps = 64, 16, 10, EPS_LEARNER
    images, labels = structured_images(n, classes=4, seed=7, size=size, noise=0.15)
    path = randomised_checkpoint(os.path.join(str(tmp_path), "densenet_random_bn.pt"), images[:8], num_classes=4)
    model = zoo.build_classifier("densenet121", num_classes=4, seed=5, weights=path, device=DEV, dtype=BF16, channels_last=True,
                                 own_dense_pointwise=True, own_dense_conv=True)
    assert sum(isinstance(m, zoo._OwnGrowthConv) for m in model.modules()) == 58
    margins, pred = zoo.fit_centroid_head(model, images.bfloat16(), labels, 4, DEV, target_margin=2.0)
    assert torch.isfinite(margins).all()
    print("fitted head on the switched network: %d of %d images classified, least margin %.3f"
          % (int((pred.cpu() == labels).sum()), n, float(margins.min())))
    x = images.to(DEV).bfloat16().contiguous()
    gen = torch.Generator().manual_seed(0)
    d0 = -1 + 2 * torch.rand(3, size, size, k, generator=gen)
    v0 = ops().l1ball_project_(torch.rand(n, k, generator=gen).to(DEV), eps).cpu()
    index = torch.arange(n, device=DEV)
    learner = engine.DictionaryLearner(d0.clone().to(DEV), v0.clone().to(DEV), eps, 0.01, "logits", False, 50.0)
    last = None
    for _ in range(20):
        ls, fl = learner.step(model, x, index)
        last = (float(ls), int(fl))
    assert torch.isfinite(learner.d).all() and torch.isfinite(learner.v).all() and last[0] == last[0]
    print("fooled after 20 steps of %d images, both switches on: %d (loss %.4f)" % (n, last[1], last[0]))
    assert last[1] >= 1, last
