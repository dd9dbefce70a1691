"""GPU: the VGG first-group kernels (adil_first3x3_pool_fwd / _bwd, csrc/adil_vgg_first.hip) through the C ABI against
the fp64 restatement of tests/vgg_first_reference.py — y, idx and gx bit for bit on the exact legs, under the derived
bounds on the gaussian leg — and the VGG11 that runs its first group on them (`own_vgg_first_conv=True` on top of
`own_vgg_conv`), when its trunk calls no library convolution, ReLU or pooling."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import vgg_first_reference as vf
from classifier_reference import BF16, CANARY, F32
from graph_tools import same_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PAD = 256                        # canary elements in front of and behind every output
IDX_CANARY = 0xAB
EPS_LEARNER = 8 / 255            # the reference CLI's radius (demo_dL_attack.py: eps 8/255, linf)


def ops():
    from dl_attack_on_imagenet_amd import ops as o
    return o


def _lib():
    return __import__("dl_attack_on_imagenet_amd._lib", fromlist=["x"]).load()


def _dev(t):
    return t.to(DEV).contiguous()


def _code(dtype):
    return {F32: 0, BF16: 1}[dtype]


def _guarded(shape, dtype):
    """An output of `shape` inside a canary-filled buffer; returns (buffer, view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), IDX_CANARY if dtype == torch.uint8 else CANARY, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n].view(shape)


def _intact(buf):
    c = IDX_CANARY if buf.dtype == torch.uint8 else CANARY
    return bool((buf[:PAD] == c).all()) and bool((buf[-PAD:] == c).all())


def _run_fwd(x, wf, bias, mean, inv_std):
    """Device tensors in; y and idx [B][H/2][W/2][64] out, each inside canaries."""
    o, lib = ops(), _lib()
    B, _, H, W = x.shape
    ybuf, y = _guarded((B, H // 2, W // 2, 64), BF16)
    ibuf, idx = _guarded((B, H // 2, W // 2, 64), torch.uint8)
    assert lib.adil_first3x3_pool_fwd(o._ptr(x), _code(x.dtype), o._ptr(wf), *mean, *inv_std, o._ptr(bias), o._ptr(y),
                                      o._ptr(idx), B, H, W, o._stream()) == 0
    torch.cuda.synchronize()
    assert _intact(ybuf) and _intact(ibuf), "forward wrote outside y or idx"
    return y, idx


def _run_bwd(g, idx, wb, inv_std, H, W, dtype):
    o, lib = ops(), _lib()
    B = g.shape[0]
    buf, gx = _guarded((B, 3, H, W), dtype)
    assert lib.adil_first3x3_pool_bwd(o._ptr(g), o._ptr(idx), o._ptr(wb), *inv_std, o._ptr(gx), _code(dtype), B, H, W,
                                      o._stream()) == 0
    torch.cuda.synchronize()
    assert _intact(buf), "gradient wrote outside gx"
    return gx


def _fwd(op, wrap=_dev):
    return _run_fwd(wrap(op.x), wrap(vf.pack_fwd(op.w)), wrap(op.bias), op.mean, op.inv_std)


def _bwd(op, idx, dtype, wrap=_dev):
    _, _, H, W = op.x.shape
    return _run_bwd(wrap(op.g), wrap(idx), wrap(vf.pack_bwd(op.w)), op.inv_std, H, W, dtype)


@pytest.mark.parametrize("row", vf.ROWS, ids=str)
def test_first_group_against_the_fp64_restatement(row):
    """Forward and input gradient of one row on the two exact legs (y, idx, gx bit for bit) and on the gaussian leg (y and
    gx under their bounds, idx by the decided / undecided rule; the gradient is fed the reference's idx).  Row names and
    operands are those of tests/test_vgg_first_cpu.py, where the emulation passes them."""
    for leg in vf.EXACT_LEGS:
        name = vf.row_name(row, leg)
        r = vf.exact_references(row, leg)
        y, idx = _fwd(r.op)
        vf.compare_fwd_exact(name, y, idx, r.fwd)
        vf.compare_bwd_exact(name, _bwd(r.op, r.fwd.idx, row[3]), r.bwd)
    name = vf.row_name(row, "gaussian")
    g = vf.gaussian_references(row)
    y, idx = _fwd(g.op)
    rf, undecided = vf.gaussian_fwd(name, y, idx, g)
    rb = vf.gaussian_bwd_ratio(_bwd(g.op, g.idx, row[3]), g.bwd)
    print(name, "max |err| / bound: fwd %.3f bwd %.3f; undecided windows %d of %d" % (rf, rb, undecided, g.idx.numel()))
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)


def _in_nan(t):
    """The same values as a view into a larger buffer: 64 NaN (bytes 0xFF for idx) directly in front of and behind it."""
    t = t.to(DEV).contiguous()
    fill = 0xFF if t.dtype == torch.uint8 else float("nan")
    buf = torch.full((t.numel() + 128,), fill, dtype=t.dtype, device=DEV)
    buf[64:64 + t.numel()] = t.reshape(-1)
    v = buf[64:64 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 0
    return v


@pytest.mark.parametrize("B,H,W", vf.OOB_ROWS)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_first_group_reads_and_writes_nothing_outside_its_operands(B, H, W, dtype):
    """x, g, idx, bias and the packed weights surrounded by NaN, the outputs by canaries: border taps and tile tails are
    predicated.  Exact legs: the result equals the restatement bit for bit and holds no NaN."""
    row = (B, H, W, dtype)
    for leg in vf.EXACT_LEGS:
        name = vf.row_name(row, leg)
        r = vf.exact_references(row, leg)
        y, idx = _fwd(r.op, _in_nan)
        gx = _bwd(r.op, r.fwd.idx, dtype, _in_nan)
        assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(gx.float()).all())
        vf.compare_fwd_exact(name, y, idx, r.fwd)
        vf.compare_bwd_exact(name, gx, r.bwd)


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("row", [(2, 18, 34, BF16), (3, 6, 10, F32)], ids=str)
def test_first_group_keeps_a_poisoned_image_to_itself(row, poison):
    """Image 1 of x (forward) and of g (gradient) filled with NaN or Inf: the other images' y, idx and gx keep their bits."""
    op = vf.gaussian_references(row).op
    y0, i0 = _fwd(op)
    gx0 = _bwd(op, i0.cpu(), row[3])
    x, g = op.x.clone(), op.g.clone()
    x[1], g[1] = poison, poison
    bad = op._replace(x=x, g=g)
    y1, i1 = _fwd(bad)
    gx1 = _bwd(bad, i0.cpu(), row[3])
    assert not bool(torch.isfinite(y1[1].float()).all()) and not bool(torch.isfinite(gx1[1].float()).all())
    keep = [b for b in range(row[0]) if b != 1]
    assert vf.same_bits(y0[keep].cpu(), y1[keep].cpu()) and torch.equal(i0[keep], i1[keep])
    assert vf.same_bits(gx0[keep].cpu(), gx1[keep].cpu())


def test_first_group_refuses_and_leaves_outputs_untouched():
    """Odd H, odd W, a NULL pointer, a misaligned pointer, a dtype code outside the two, sizes outside the limits:
    ADIL_EINVAL and canary-filled outputs untouched.  These calls launch nothing."""
    o, lib = ops(), _lib()
    big = torch.zeros(1 << 16, dtype=BF16, device=DEV)
    tab = torch.zeros(64, dtype=F32, device=DEV)
    out = torch.full((1 << 16,), CANARY, dtype=BF16, device=DEV)
    iout = torch.full((1 << 16,), IDX_CANARY, dtype=torch.uint8, device=DEV)
    P, S = o._ptr, o._stream
    nm = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)

    def fwd(x, dt, w, bias, y, idx, B, H, W):
        return lib.adil_first3x3_pool_fwd(x, dt, w, *nm, bias, y, idx, B, H, W, S())

    def bwd(g, idx, w, gx, dt, B, H, W):
        return lib.adil_first3x3_pool_bwd(g, idx, w, *nm[3:], gx, dt, B, H, W, S())

    for (B, H, W, dt) in [(2, 7, 8, 1), (2, 8, 7, 1), (2, 1, 8, 1), (0, 8, 8, 1), (-1, 8, 8, 1), (2, 0, 8, 1), (2, 8, 0, 1),
                          (2, 8, -8, 1), (2, 8, 8, 2), (2, 8, 8, -1), (65536, 2, 2, 1), (2, 32768, 32768, 1)]:
        assert fwd(P(big), dt, P(big), P(tab), P(out), P(iout), B, H, W) == EINVAL, (B, H, W, dt)
        assert bwd(P(big), P(iout), P(big), P(out), dt, B, H, W) == EINVAL, (B, H, W, dt)
    a = (P(big), P(big), P(tab), P(out), P(iout))
    for i in range(5):                                                 # each NULL pointer of the forward
        v = [None if j == i else p for j, p in enumerate(a)]
        assert fwd(v[0], 1, v[1], v[2], v[3], v[4], 2, 8, 8) == EINVAL, i
    a = (P(big), P(iout), P(big), P(out))
    for i in range(4):                                                 # and of the gradient
        v = [None if j == i else p for j, p in enumerate(a)]
        assert bwd(v[0], v[1], v[2], v[3], 1, 2, 8, 8) == EINVAL, i
    assert fwd(P(big), 1, P(big[4:]), P(tab), P(out), P(iout), 2, 8, 8) == EINVAL                      # misaligned w_fwd
    assert fwd(P(big), 1, P(big), P(tab[1:]), P(out), P(iout), 2, 8, 8) == EINVAL                      # misaligned bias
    assert fwd(P(big), 1, P(big), P(tab), P(out[4:]), P(iout), 2, 8, 8) == EINVAL                      # misaligned y
    assert fwd(P(big), 1, P(big), P(tab), P(out), P(iout[8:]), 2, 8, 8) == EINVAL                      # misaligned idx
    assert fwd(P(big[1:]), 0, P(big), P(tab), P(out), P(iout), 2, 8, 8) == EINVAL                      # fp32 x at 2 bytes
    assert bwd(P(big[4:]), P(iout), P(big), P(out), 1, 2, 8, 8) == EINVAL                              # misaligned g
    assert bwd(P(big), P(iout[4:]), P(big), P(out), 1, 2, 8, 8) == EINVAL                              # misaligned idx
    assert bwd(P(big), P(iout), P(big[4:]), P(out), 1, 2, 8, 8) == EINVAL                              # misaligned w_bwd
    assert bwd(P(big), P(iout), P(big), P(out[1:]), 0, 2, 8, 8) == EINVAL                              # fp32 gx at 2 bytes
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and bool((iout == IDX_CANARY).all())


AUTOGRAD_ROWS = [(2, 14, 14), (3, 6, 10), (2, 18, 34)]


@pytest.mark.parametrize("b,h,w", AUTOGRAD_ROWS)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_autograd_function_equals_the_c_abi_bitwise(b, h, w, dtype):
    """ops.first_conv3x3_pool on the attack's NCHW tensor: the very bits of the C-ABI calls, the output in channels_last
    storage, only idx saved, the gradient in x's dtype and layout."""
    o = ops()
    op = vf.operands("autograd/%s" % ((b, h, w),), "gaussian", b, h, w, dtype)
    want_y, want_idx = _fwd(op)
    want_gx = _bwd(op, want_idx.cpu(), dtype)
    wf, wb = o.pack_first3x3_pool_weights(_dev(op.w))
    assert torch.equal(wf.reshape(64, 3, 4, 4), _dev(vf.pack_fwd(op.w))) and torch.equal(wb.reshape(3, 9, 64), _dev(vf.pack_bwd(op.w)))
    args = (wf, wb, _dev(op.bias), op.mean, op.inv_std)
    x = _dev(op.x).requires_grad_(True)
    y = o.first_conv3x3_pool(x, *args)
    assert y.shape == (b, 64, h // 2, w // 2) and y.dtype == BF16 and y.permute(0, 2, 3, 1).is_contiguous()
    assert vf.same_bits(y.detach().permute(0, 2, 3, 1).cpu(), want_y.cpu())
    saved = [t for t in y.grad_fn.saved_tensors if t.dtype == torch.uint8]
    assert len(saved) == 1 and torch.equal(saved[0], want_idx)
    assert not any(t.shape == y.shape or t.shape == x.shape for t in y.grad_fn.saved_tensors)     # neither x nor y is kept
    (gx,) = torch.autograd.grad(y, x, _dev(op.g).permute(0, 3, 1, 2))
    assert gx.shape == x.shape and gx.dtype == dtype and gx.is_contiguous()
    assert vf.same_bits(gx.cpu(), want_gx.cpu())
    for bad in (lambda: o.first_conv3x3_pool(x.double(), *args), lambda: o.first_conv3x3_pool(x[:, :2], *args),
                lambda: o.first_conv3x3_pool(x[:, :, 1:], *args), lambda: o.first_conv3x3_pool(x[:, :, :, 1:], *args),
                lambda: o.first_conv3x3_pool(x, wf, wb, args[2].double(), op.mean, op.inv_std),
                lambda: o.first_conv3x3_pool(x, wf.float(), wb, args[2], op.mean, op.inv_std)):
        with pytest.raises(ValueError):
            bad()


def test_first_group_in_a_captured_graph():
    """Forward + input gradient captured in a graph and replayed on two input sets equals the eager result bit for bit: the
    calls launch on the capturing stream and neither synchronise nor allocate outside the allocator."""
    o = ops()
    b, h, w = 4, 18, 34
    sets = [vf.operands("graph/%d" % i, "gaussian", b, h, w, BF16) for i in range(2)]
    wf, wb = o.pack_first3x3_pool_weights(_dev(sets[0].w))
    args = (wf, wb, _dev(sets[0].bias), sets[0].mean, sets[0].inv_std)
    nchw = lambda g: _dev(g).permute(0, 3, 1, 2)

    def run(x, g):
        y = o.first_conv3x3_pool(x, *args)
        (gx,) = torch.autograd.grad(y, x, g)
        return dict(y=y.detach(), gx=gx)

    eager = [{k: t.clone() for k, t in run(_dev(q.x).requires_grad_(True), nchw(q.g)).items()} for q in sets]
    assert float(eager[0]["y"].abs().max()) > 0 and float(eager[0]["gx"].abs().max()) > 0
    xs = _dev(sets[0].x).clone().requires_grad_(True)
    gs = nchw(sets[0].g).clone(memory_format=torch.preserve_format)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(xs, gs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(xs, gs)
    for q, want in zip(sets, eager):
        with torch.no_grad():
            xs.copy_(_dev(q.x))
            gs.copy_(nchw(q.g))
        graph.replay()
        torch.cuda.synchronize()
        same_state(out, want, ("y", "gx"))


def test_first_group_is_bitwise_across_processes():
    """Two fresh child processes, one after the other (the second only if the first exited 0), each under `timeout`:
    byte-identical y, idx and gx for three rows."""
    child = os.path.join(ROOT, "tests", "vgg_first_child.py")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
    outs = []
    for _ in range(2):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, child], env=env, capture_output=True, text=True,
                           timeout=270, cwd=ROOT)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("hash ")]
        assert len(lines) == 3 * len(vf.HASH_ROWS), r.stdout[-2000:]
        outs.append(lines)
    for a, b in zip(*outs):
        assert a == b, (a, b)


# ------------------------------------------------------------------------------------------------------------- network
def vgg_checkpoint(path, seed=5, num_classes=1000):
    """The construction of tests/test_gpu_vgg_conv.py, restated: a seeded VGG11 state_dict with kaiming fan-out
    convolution weights and biases N(0, 0.1), so that the bias path is under test."""
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
    assert g.shape == x.shape and g.dtype == x.dtype
    return logits.detach(), g.detach().float()


@pytest.fixture(scope="module")
def networks(tmp_path_factory):
    """What the network cases share, built once and left unchanged: the fp32 network, the plain bf16 network, the one with
    `own_vgg_conv` alone and the one with `own_vgg_first_conv` on top (16 classes)."""
    from dl_attack_on_imagenet_amd import zoo
    path = vgg_checkpoint(os.path.join(str(tmp_path_factory.mktemp("vggfirst")), "vgg11_kaiming.pt"), num_classes=16)
    kw = dict(num_classes=16, seed=5, weights=path, device=DEV)
    fp32 = zoo.build_classifier("vgg11", **kw)
    kw.update(dtype=BF16, channels_last=True)
    return (fp32, zoo.build_classifier("vgg11", **kw), zoo.build_classifier("vgg11", own_vgg_conv=True, **kw),
            zoo.build_classifier("vgg11", own_vgg_conv=True, own_vgg_first_conv=True, **kw))


def _count(mp, obj, name, log, key=lambda a: None):
    real = getattr(obj, name)
    mp.setattr(obj, name, lambda *a, **k: (log.append((name, key(a))), real(*a, **k))[1])


def _network_case(networks, size, fp32_x=False):
    """The existing criterion: against the fp32 network, mean |logit error| and relative input-gradient error at most
    1.5 x the plain bf16 network's own."""
    from structured import structured_images
    fp32, plain, _, own = networks
    images, _ = structured_images(2, classes=2, seed=3, size=size)
    x = images.to(DEV)
    lr, gr = _forward_and_gradient(fp32, x)
    l0, g0 = _forward_and_gradient(plain, x.bfloat16())
    l1, g1 = _forward_and_gradient(own, x if fp32_x else x.bfloat16())
    rel = lambda g: float((g - gr).norm() / gr.norm())
    e0, e1, r0, r1 = float((l0 - lr).abs().mean()), float((l1 - lr).abs().mean()), rel(g0), rel(g1)
    print("VGG11 at %d x %d (%s x): mean |logit error| vs fp32: plain bf16 %.5f, both switches %.5f; input gradient "
          "relative error vs fp32: plain %.4f both switches %.4f" % (size, size, "fp32" if fp32_x else "bf16", e0, e1, r0, r1))
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all() and g1.shape == x.shape
    assert float(l1.abs().max()) > 0 and float(g1.abs().max()) > 0 and float(gr.abs().max()) > 0
    assert e1 <= 1.5 * e0, (e0, e1)
    assert r1 <= 1.5 * r0, (r0, r1)
    return own, x


def _trunk_calls(monkeypatch, model, x):
    o, log = ops(), []
    with monkeypatch.context() as mp:
        _count(mp, F, "conv2d", log)
        _count(mp, F, "max_pool2d", log)
        _count(mp, F, "relu", log)
        _count(mp, o, "first_conv3x3_pool", log, lambda a: a[0].shape[3])
        _count(mp, o, "bias_relu_pool2", log, lambda a: a[0].shape[3])
        with torch.no_grad():
            model(x)
    return lambda n: [k for name, k in log if name == n]


def test_vgg11_trunk_calls_no_library_kernel(networks, monkeypatch):
    """Both switches on 2 structured images at 128 x 128: F.conv2d and F.max_pool2d are never reached, F.relu twice (the
    classifier), ops.first_conv3x3_pool once, bias_relu_pool2 at W = 64, 32, 16, 8 only; the criterion holds."""
    own, x = _network_case(networks, 128)
    calls = _trunk_calls(monkeypatch, own, x.bfloat16())
    assert calls("conv2d") == [] and calls("max_pool2d") == [] and len(calls("relu")) == 2
    assert calls("first_conv3x3_pool") == [128] and calls("bias_relu_pool2") == [64, 32, 16, 8]


def test_vgg11_takes_an_fp32_stream(networks):
    _network_case(networks, 128, fp32_x=True)


def test_vgg11_first_group_stays_on_the_kernel_at_126(networks, monkeypatch):
    """126 x 126: the grids are 126, 63, 31, 15, 7, so the four later pooled groups meet odd grids and keep their original
    modules (one F.conv2d and one F.max_pool2d each), while the first group stays on the new kernel."""
    own, x = _network_case(networks, 126)
    calls = _trunk_calls(monkeypatch, own, x.bfloat16())
    assert calls("first_conv3x3_pool") == [126] and calls("bias_relu_pool2") == []
    assert len(calls("conv2d")) == 4 and len(calls("max_pool2d")) == 4


class _Memo:
    """Makes F.conv2d and F.linear repeat themselves while it is in force: a call whose tensor arguments hold the bytes
    of an earlier call's (same dtype, shape and remaining arguments) gets a copy of that call's result.  The library's bf16
    convolutions do not give the same bits call to call on every box; with this two networks that make the same library
    calls on the same operands give the same bits, and two that do not, do not."""

    def __init__(self, mp):
        import hashlib
        self.store, self.hits = {}, 0

        def key(v):
            if isinstance(v, torch.Tensor):
                t = v.detach().contiguous()
                return (str(t.dtype), tuple(t.shape), hashlib.sha256(t.view(torch.uint8).cpu().numpy().tobytes()).hexdigest())
            return repr(v)

        for name in ("conv2d", "linear"):
            real = getattr(F, name)

            def call(*a, _name=name, _real=real, **k):
                kk = (_name,) + tuple(key(v) for v in a) + tuple((n, key(v)) for n, v in sorted(k.items()))
                if kk in self.store:
                    self.hits += 1
                else:
                    self.store[kk] = _real(*a, **k).clone()
                return self.store[kk].clone()

            mp.setattr(F, name, call)


def test_vgg11_first_group_falls_back_at_127(networks, monkeypatch):
    """127 x 127: the first group falls back to torch's normalisation and the route of `own_vgg_conv` alone, and the output
    equals that network's.  The grids 127, 63, 31, 15, 7 are all odd, so five library convolutions and five pools follow.
    Three comparisons, none of which can be switched off:
      - the tensor that reaches the first convolution has the bits of that network's `Normalize` output;
      - with F.conv2d and F.linear made to repeat themselves (`_Memo`: the library's bf16 convolutions do not on every
        box), the logits are equal BIT FOR BIT, and every library call of the second network is one the first made;
      - on the library as it is, max |got - want| <= 8 max(max |want - again|, one bf16 ulp of the largest logit), `again`
        being the own_vgg_conv-only network's own second call: the noise between two of its calls, not a tolerance of ours."""
    from structured import structured_images
    _, _, conv_only, own = networks
    images, _ = structured_images(2, classes=2, seed=3, size=127)
    x = images.to(DEV).bfloat16()
    calls = _trunk_calls(monkeypatch, own, x)
    assert calls("first_conv3x3_pool") == [] and len(calls("conv2d")) == 5 and len(calls("max_pool2d")) == 5
    seen = {}
    hooks = [net.features[0].register_forward_pre_hook(lambda m, a, k=k: seen.__setitem__(k, a[0].detach().clone()))
             for k, net in (("own", own[0]), ("conv_only", conv_only[1]))]
    with torch.no_grad():
        for _ in range(2):                                 # both networks warmed at this size
            got, want = own(x), conv_only(x)
        again = conv_only(x)
    for h in hooks:
        h.remove()
    assert seen["own"].shape == (2, 3, 127, 127) and vf.same_bits(seen["own"].cpu(), seen["conv_only"].cpu())
    with monkeypatch.context() as mp, torch.no_grad():
        memo = _Memo(mp)
        want_m = conv_only(x)
        made = len(memo.store)
        got_m = own(x)
    assert made == 8 and len(memo.store) == 8 and memo.hits == 8, (made, len(memo.store), memo.hits)   # 5 conv2d + 3 linear
    assert float(want_m.float().abs().max()) > 0 and torch.equal(got_m, want_m)
    diff = lambda a, b: float((a.float() - b.float()).abs().max())
    ulp = 2.0 ** -7 * float(want.float().abs().max())
    d, noise = diff(got, want), diff(want, again)
    print("127 x 127: max |logit difference| to the own_vgg_conv-only network %.3g; that network against its own second call "
          "%.3g; one bf16 ulp of the largest logit %.3g" % (d, noise, ulp))
    assert d <= 8 * max(noise, ulp), (d, noise, ulp)


def test_learner_steps_against_vgg11_reported(networks):
    """Reported leg, finite values only: 10 learner steps (bf16 streams, 8 structured images at 128 x 128, K = 10) against
    the VGG11 with both switches; the loss and the number of fooled images are printed."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import engine
    model = networks[3]
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
    print("fooled after 10 steps of %d images, both switches on: %d (loss %.4f)" % (n, last[1], last[0]))
