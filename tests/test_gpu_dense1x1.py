"""GPU: the pre-activated pointwise kernels (adil_dense1x1_fwd / adil_dense1x1_bwd, csrc/adil_dense1x1.hip) through the C
ABI against the fp64 restatement of tests/dense1x1_reference.py — bit for bit on the exact legs, under the derived
elementwise bound on the gaussian leg — and the DenseNet-121 that runs its 61 pre-activated 1x1 layers on them
(`own_dense_pointwise=True`)."""
import os
import subprocess
import sys

import pytest
import torch

import dense1x1_reference as dref
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
    return None if t is None else t.to(DEV).contiguous()


def _run_fwd(x, pscale, pshift, w, scale, shift, act):
    """Device tensors in, y [M][N] out; canary rows behind y."""
    o, lib = ops(), _lib()
    M, K, N = x.shape[0], x.shape[1], w.shape[0]
    y = torch.full((M + PAD, N), CANARY, dtype=BF16, device=DEV)
    assert lib.adil_dense1x1_fwd(o._ptr(x), o._ptr(pscale), o._ptr(pshift), o._ptr(w), o._ptr(scale), o._ptr(shift), o._ptr(y),
                                 M, K, N, act, o._stream()) == 0
    torch.cuda.synchronize()
    assert bool((y[M:] == CANARY).all()), "forward wrote past the end of y"
    return y[:M]


def _run_bwd(g, y, scale, wt, xin, pscale, pshift, act):
    o, lib = ops(), _lib()
    M, N, K = g.shape[0], g.shape[1], wt.shape[0]
    gx = torch.full((M + PAD, K), CANARY, dtype=BF16, device=DEV)
    assert lib.adil_dense1x1_bwd(o._ptr(g), o._ptr(y), o._ptr(scale), o._ptr(wt), o._ptr(xin), o._ptr(pscale), o._ptr(pshift),
                                 o._ptr(gx), M, K, N, act, o._stream()) == 0
    torch.cuda.synchronize()
    assert bool((gx[M:] == CANARY).all()), "gradient wrote past the end of gx"
    return gx[:M]


def _fwd(op, act):
    return _run_fwd(_dev(op.x), _dev(op.pscale), _dev(op.pshift), _dev(op.w), _dev(op.scale), _dev(op.shift), act)


def _bwd(op, y, act):
    return _run_bwd(_dev(op.g), _dev(y), _dev(op.scale), _dev(op.wt), _dev(op.x), _dev(op.pscale), _dev(op.pshift), act)


@pytest.mark.parametrize("row", dref.ROWS, ids=str)
def test_dense1x1_against_the_fp64_restatement(row):
    """Forward and input gradient of one row on its exact leg (clamp set with act 1, rounding set with act 0), bit for bit,
    and on the gaussian leg under the derived bound.  Row names and operands are those of tests/test_dense1x1_cpu.py,
    where the emulation passes them and every premise is asserted on the reference alone."""
    M, K, N, act = row
    name = dref.row_name(*row)
    exact, _ = dref.legs_of(act)
    r = dref.reference_row(name, exact, M, K, N, act)
    dref.compare_exact(name + "/" + exact + "/fwd", _fwd(r.ops, act), r.fwd)
    dref.compare_exact(name + "/" + exact + "/bwd", _bwd(r.ops, r.y, act), r.bwd)
    r = dref.reference_row(name, "gaussian", M, K, N, act)
    rf = dref.gaussian_ratio(_fwd(r.ops, act).cpu(), r.fwd)
    rb = dref.gaussian_ratio(_bwd(r.ops, r.y, act).cpu(), r.bwd)
    print(name, "gaussian max |err| / bound: fwd %.3f bwd %.3f" % (rf, rb))
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)


def _in_nan(t):
    """The same values as a view into a larger buffer of NaN: 64 NaN directly in front of and behind the operand."""
    t = t.to(DEV).contiguous()
    buf = torch.full((t.numel() + 128,), float("nan"), dtype=t.dtype, device=DEV)
    buf[64:64 + t.numel()] = t.reshape(-1)
    v = buf[64:64 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 0 and bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all())
    return v


@pytest.mark.parametrize("M,K,N", dref.NAN_ROWS)
def test_dense1x1_reads_nothing_outside_its_operands(M, K, N):
    """x, w, g, wt, xin and the [K] / [N] tables surrounded by NaN: the K tail (K % 16 = 8, K % 64 != 0), the N tail
    (N % 32 = 8) and the tables' tails are clipped and zero-filled, not read from the neighbouring row or from behind the
    operand.  Exact legs: the result equals the plain call and the restatement bit for bit and holds no NaN."""
    for act in (1, 0):
        name = dref.row_name(M, K, N, act)
        exact, _ = dref.legs_of(act)
        r = dref.reference_row(name, exact, M, K, N, act)
        op = r.ops
        plain_y, plain_gx = _fwd(op, act), _bwd(op, r.y, act)
        got_y = _run_fwd(_in_nan(op.x), _in_nan(op.pscale), _in_nan(op.pshift), _in_nan(op.w), _in_nan(op.scale),
                         _in_nan(op.shift), act)
        got_gx = _run_bwd(_in_nan(op.g), _dev(r.y), _in_nan(op.scale), _in_nan(op.wt), _in_nan(op.x), _in_nan(op.pscale),
                          _in_nan(op.pshift), act)
        assert not bool(torch.isnan(got_y).any()) and not bool(torch.isnan(got_gx).any())
        assert torch.equal(got_y.view(torch.int16), plain_y.view(torch.int16))
        assert torch.equal(got_gx.view(torch.int16), plain_gx.view(torch.int16))
        dref.compare_exact(name + "/fwd", got_y, r.fwd)
        dref.compare_exact(name + "/bwd", got_gx, r.bwd)


def test_dense1x1_refuses_and_leaves_outputs_untouched():
    """K = 12, N = 20, K = 2056, N = 2056, M = 0, act 2 / -1, K = 0, K = 4, every NULL mandatory pointer, NULL y with act 1,
    misaligned bf16 pointers and misaligned tables: ADIL_EINVAL, canaries intact."""
    o, lib = ops(), _lib()
    big = torch.zeros(64 * 2064, dtype=BF16, device=DEV)
    tab = torch.zeros(2064, dtype=torch.float32, device=DEV)
    out = torch.full((64 * 2064,), CANARY, dtype=BF16, device=DEV)
    P, S = o._ptr, o._stream
    odd = lambda t: t.data_ptr() + 2                          # a table address that is no multiple of 4

    def fwd(x, ps, pb, w, sc, sh, y, M, K, N, act):
        return lib.adil_dense1x1_fwd(x, ps, pb, w, sc, sh, y, M, K, N, act, S())

    def bwd(g, y, sc, wt, xin, ps, pb, gx, M, K, N, act):
        return lib.adil_dense1x1_bwd(g, y, sc, wt, xin, ps, pb, gx, M, K, N, act, S())

    good_f = [P(big), P(tab), P(tab), P(big), P(tab), P(tab), P(out)]
    good_b = [P(big), P(big), P(tab), P(big), P(big), P(tab), P(tab), P(out)]
    for (M, K, N, act) in [(64, 12, 16, 0), (64, 16, 20, 0), (64, 2056, 16, 0), (64, 16, 2056, 1), (0, 16, 16, 1), (64, 16, 16, 2),
                           (64, 16, 16, -1), (64, 0, 16, 0), (64, 4, 8, 1), (64, 8, 4, 1)]:
        assert fwd(*good_f, M, K, N, act) == EINVAL, (M, K, N, act)
        assert bwd(*good_b, M, K, N, act) == EINVAL, (M, K, N, act)
    for i in range(len(good_f)):                              # every pointer of the forward is mandatory
        a = list(good_f)
        a[i] = None
        assert fwd(*a, 64, 16, 16, 0) == EINVAL, i
    for i in range(len(good_b)):                              # and of the gradient, with act 1
        a = list(good_b)
        a[i] = None
        assert bwd(*a, 64, 16, 16, 1) == EINVAL, i
    for i in (0, 3, 6):                                       # misaligned x, w, y
        a = list(good_f)
        a[i] = P(big[4:]) if i != 6 else P(out[4:])
        assert fwd(*a, 64, 16, 16, 0) == EINVAL, i
    for i in (1, 2, 4, 5):                                    # misaligned tables
        a = list(good_f)
        a[i] = odd(tab)
        assert fwd(*a, 64, 16, 16, 0) == EINVAL, i
    for i in (0, 1, 3, 4, 7):                                 # misaligned g, y, wt, xin, gx
        a = list(good_b)
        a[i] = P(big[4:]) if i != 7 else P(out[4:])
        assert bwd(*a, 64, 16, 16, 1) == EINVAL, i
    for i in (2, 5, 6):
        a = list(good_b)
        a[i] = odd(tab)
        assert bwd(*a, 64, 16, 16, 1) == EINVAL, i
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    # the accepted forms: tables at a 4-byte (not 16-byte) address; y NULL without a ReLU (it is not read)
    assert fwd(P(big), P(tab[1:]), P(tab[3:]), P(big), P(tab[1:]), P(tab[2:]), P(out), 64, 16, 16, 1) == 0
    a = list(good_b)
    a[1] = None
    assert bwd(*a, 64, 16, 16, 0) == 0
    torch.cuda.synchronize()
    assert bool((out[:64 * 16] == 0).all()) and bool((out[64 * 16:] == CANARY).all())


AUTOGRAD_ROWS = [(2, 14, 14, 96, 128, 1), (3, 7, 5, 256, 128, 0), (2, 9, 11, 24, 40, 1)]


def _nchw(t, b, h, w):
    return t.to(DEV).reshape(b, h, w, -1).permute(0, 3, 1, 2)


def _args(op):
    return (_dev(op.pscale), _dev(op.pshift), _dev(op.w), _dev(op.wt), _dev(op.scale), _dev(op.shift))


@pytest.mark.parametrize("b,h,w,k,n,act", AUTOGRAD_ROWS)
def test_autograd_function_equals_the_c_abi_bitwise(b, h, w, k, n, act):
    """ops.dense1x1_conv on NCHW-shaped channels_last tensors: no copies in or out and the very bits of the C-ABI calls
    (the backward reads the saved x and y); ValueError on a wrong dtype, shape or layout."""
    o = ops()
    op = dref.operands("autograd/%s" % ((b, h, w, k, n),), "gaussian", b * h * w, k, n)
    want_y = _fwd(op, act)
    want_gx = _bwd(op, want_y if act else None, act)
    x = _nchw(op.x, b, h, w).requires_grad_(True)
    args = _args(op)
    y = o.dense1x1_conv(x, *args, bool(act))
    assert y.shape == (b, n, h, w) and y.dtype == BF16 and y.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(y.detach().permute(0, 2, 3, 1).reshape(-1, n).view(torch.int16), want_y.view(torch.int16))
    saved = [t.data_ptr() for t in y.grad_fn.saved_tensors]
    assert x.data_ptr() in saved and y.data_ptr() in saved           # x and y themselves, not copies
    g = _nchw(op.g, b, h, w)
    (gx,) = torch.autograd.grad(y, (x,), g)
    assert gx.shape == x.shape and gx.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(gx.permute(0, 2, 3, 1).reshape(-1, k).view(torch.int16), want_gx.view(torch.int16))
    with pytest.raises(ValueError):
        o.dense1x1_conv(x.float(), *args, bool(act))
    with pytest.raises(ValueError):
        o.dense1x1_conv(x[:, :k - 4], *args, bool(act))
    with pytest.raises(ValueError):
        o.dense1x1_conv(x, args[0].double(), *args[1:], bool(act))
    with pytest.raises(ValueError):
        o.dense1x1_conv(x, args[0], args[1][:-1], *args[2:], bool(act))
    with pytest.raises(ValueError):
        o.dense1x1_conv(x, args[0], args[1], args[2].t(), *args[3:], bool(act))
    with pytest.raises(ValueError):                                  # NCHW-contiguous x: it would have to be copied
        o.dense1x1_conv(x.detach().contiguous(), *args, bool(act))


def test_dense1x1_in_a_captured_graph():
    """One layer's forward + input gradient captured in a graph and replayed (on fresh inputs copied into the captured
    buffers) equals the eager result bit for bit: the calls launch on the capturing stream and neither synchronise nor
    allocate outside the allocator."""
    o = ops()
    b, h, w, k, n = 4, 14, 14, 416, 128
    op = dref.operands("graph", "gaussian", b * h * w, k, n)
    op2 = dref.operands("graph/2", "gaussian", b * h * w, k, n)
    args = _args(op)

    def run(x, g):
        y = o.dense1x1_conv(x, *args, True)
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


def test_dense1x1_is_bitwise_across_processes():
    """Two fresh child processes, one after the other (the second only if the first exited 0), each under `timeout`:
    byte-identical y and gx for three rows."""
    child = os.path.join(ROOT, "tests", "dense1x1_child.py")
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
    """The recipe of tests/test_gpu_pointwise8.randomised_checkpoint, restated for DenseNet-121: a seeded state_dict with
    randomised BatchNorm statistics and affine maps.
    images None: statistics drawn around the initial 0 / 1, gamma of BOTH signs ((0.7 + 0.6 u) with a random sign: the
      pscale / scale tables take both signs), for the precision comparisons.
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


def test_densenet_on_own_dense_pointwise_kernels(tmp_path):
    """`own_dense_pointwise=True` on 4 structured images at 64 x 64, a checkpoint with randomised BatchNorm statistics and
    gamma of both signs: each of the 61 rewritten layers against the restatement applied to its actual input (gaussian
    bound, ratio printed), the layers seen in network order, the logits against the fp32 network within the bf16 depth
    bound of 121 layers, and the input gradient no further from the fp32 network's than 1.5 x the distance of the plain
    bf16 network (the parent path).
    Recorded on an MI355X: the 61 layers at 0.744-0.989 of their elementwise bound (a correctly rounded bf16 result uses all
    of the 2^-8 |r| term); mean |logit error| 0.00536 off / 0.00278 own_dense_pointwise, rms logit 0.6155, bound 0.02645;
    input-gradient relative error 0.1399 off / 0.1317 own_dense_pointwise (the library
    convolutions are not reproducible call to call: a second run gave 0.00533 / 0.00278 and 0.1402 / 0.1318)."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import zoo
    size = 64
    images, _ = structured_images(4, classes=4, seed=3, size=size)
    path = randomised_checkpoint(os.path.join(str(tmp_path), "densenet_random_bn.pt"))
    kw = dict(num_classes=1000, seed=5, weights=path, device=DEV)
    ref = zoo.build_classifier("densenet121", **kw)
    kw.update(dtype=BF16, channels_last=True)
    off = zoo.build_classifier("densenet121", **kw)
    own = zoo.build_classifier("densenet121", own_dense_pointwise=True, **kw)
    x = images.to(DEV)
    seen, held = [], {}
    flat = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1])

    def restate(mod, conv, xin, out, act):
        assert xin.dtype == BF16 and xin.is_contiguous(memory_format=torch.channels_last)
        o = dref.d1_fwd(Arith(), flat(xin), mod.pscale, mod.pshift, conv.weight.detach().reshape(mod.cout, mod.cin), mod.scale,
                        mod.shift, act)
        seen.append((mod.cin, mod.cout, xin.shape[2], act, dref.gaussian_ratio(flat(out), o)))

    handles = []
    for m in own.modules():
        if isinstance(m, zoo._OwnDenseLayer):
            # the kernel's output is conv2's input; its input is the concatenation of the layer's arguments
            handles.append(m.conv2.register_forward_hook(lambda mod, args, out, lay=m: held.__setitem__(lay, args[0])))
            handles.append(m.register_forward_hook(lambda mod, args, out: restate(
                mod, mod.conv1, torch.cat(args[0], 1), held.pop(mod), 1)))
        elif isinstance(m, zoo._OwnTransition):
            handles.append(m.pool.register_forward_hook(lambda mod, args, out, lay=m: held.__setitem__(lay, args[0])))
            handles.append(m.register_forward_hook(lambda mod, args, out: restate(mod, mod.conv, args[0], held.pop(mod), 0)))
    assert len(handles) == 2 * 61
    l1, g1 = _forward_and_gradient(own, x.bfloat16())
    for h in handles:
        h.remove()
    l0, g0 = _forward_and_gradient(off, x.bfloat16())
    # the network's list at this size: every grid scales with the image (56, 28, 14, 7 at 224 -> 16, 8, 4, 2 at 64)
    assert [s[:4] for s in seen] == [(k, n, h * size // 224, a) for k, n, h, a in dref.DENSENET_LAYERS_ALL61]
    for k, n, h, act, ratio in seen:
        print("layer %4d -> %4d at %3d x %3d act %d: max |err| / bound %.3f" % (k, n, h, h, act, ratio))
        assert ratio <= 1.0, (k, n, h, act, ratio)
    lr, gr = _forward_and_gradient(ref, x)
    rms = float(lr.square().mean().sqrt())
    bound = _bf16_depth_bound(121) * rms
    rel = lambda g: float((g - gr).norm() / gr.norm())
    e0, e1 = (float((l - lr).abs().mean()) for l in (l0, l1))
    r0, r1 = rel(g0), rel(g1)
    print("logit error vs fp32: off %.5f own_dense_pointwise %.5f, rms %.4f, bound %.5f; input gradient relative error vs "
          "fp32: off %.4f own_dense_pointwise %.4f" % (e0, e1, rms, bound, r0, r1))
    assert float(gr.abs().max()) > 0 and float(g1.abs().max()) > 0
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all() and g1.shape == x.shape
    assert e1 <= bound, (e0, e1, rms)
    assert r1 <= 1.5 * r0, (r0, r1)


def test_learner_steps_against_densenet_reported(tmp_path):
    """Reported leg, sanity bounds only: 20 learner steps (bf16 streams, 16 structured images at 64 x 64, K = 10) against
    DenseNet-121 with the switch on and a head fitted by `fit_centroid_head` ON the switched network.  All values finite,
    at least one image fooled; the count is printed.
    Recorded on an MI355X, two runs (the library convolutions are not reproducible call to call and the random-weight
    network amplifies it): the fitted head classifies 16 of 16 images, least margin 1.480 / 1.525; 3 / 1 images fooled
    after 20 steps, loss -2.6165 / 0.4463."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import engine, zoo
    size, n, k, eps = 64, 16, 10, EPS_LEARNER
    images, labels = structured_images(n, classes=4, seed=7, size=size, noise=0.15)
    path = randomised_checkpoint(os.path.join(str(tmp_path), "densenet_random_bn.pt"), images[:8], num_classes=4)
    model = zoo.build_classifier("densenet121", num_classes=4, seed=5, weights=path, device=DEV, dtype=BF16, channels_last=True,
                                 own_dense_pointwise=True)
    assert sum(isinstance(m, (zoo._OwnDenseLayer, zoo._OwnTransition)) for m in model.modules()) == 61
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
    print("fooled after 20 steps of %d images, switch on: %d (loss %.4f)" % (n, last[1], last[0]))
    assert last[1] >= 1, last
