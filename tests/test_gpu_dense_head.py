"""GPU: the pooled head kernels behind a BatchNorm + ReLU (adil_bn_pool_head_fwd / adil_bn_pool_head_bwd, csrc/adil_head.hip)
through the C ABI against the restatement of tests/dense_head_reference.py — bit for bit on the exact leg, under the derived
elementwise bounds on the gaussian leg — `ops.bn_pool_head` under autograd and in a captured graph, and the DenseNet-121 that
runs norm5 + ReLU + pooling + classifier on them (`own_dense_head=True | "inference"`), alone and with the five dense
switches, when no library call is left in the network."""
import os
import subprocess
import sys
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

import dense_head_reference as dref
from classifier_reference import BF16, CANARY, F32

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PAD = 256                        # canary elements in front of and behind every output
FIVE = dict(own_dense_pointwise=True, own_dense_conv=True, own_dense_block=True, own_dense_transition=True, own_dense_stem=True)


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
    return t.to(DEV).contiguous()


def _guarded(shape, dtype):
    """An output of `shape` inside a canary-filled buffer; returns (buffer, view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), CANARY, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n].view(shape)


def _intact(buf):
    return bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all())


def _run_fwd(x, pscale, pshift, wt, bias):
    """Device tensors in (x [B][HW][C] bf16, tables [C], wt [C][N], bias [N]); pooled and logits out, canaries around both."""
    o, lib = ops(), _lib()
    B, HW, C = x.shape
    N = wt.shape[1]
    pbuf, pooled = _guarded((B, C), F32)
    lbuf, logits = _guarded((B, N), F32)
    assert lib.adil_bn_pool_head_fwd(o._ptr(x), o._ptr(pscale), o._ptr(pshift), o._ptr(wt), o._ptr(bias), o._ptr(pooled),
                                     o._ptr(logits), B, HW, C, N, o._stream()) == 0
    torch.cuda.synchronize()
    assert _intact(pbuf) and _intact(lbuf), "forward wrote outside pooled / logits"
    return pooled, logits


def _run_bwd(g, w, x, pscale, pshift):
    o, lib = ops(), _lib()
    B, HW, C = x.shape
    N = g.shape[1]
    pbuf, gpooled = _guarded((B, C), F32)
    xbuf, gx = _guarded((B, HW, C), BF16)
    assert lib.adil_bn_pool_head_bwd(o._ptr(g), o._ptr(w), o._ptr(x), o._ptr(pscale), o._ptr(pshift), o._ptr(gpooled),
                                     o._ptr(gx), B, HW, C, N, o._stream()) == 0
    torch.cuda.synchronize()
    assert _intact(pbuf) and _intact(xbuf), "gradient wrote outside gpooled / gx"
    return gpooled, gx


def _run(op, wrap=_dev):
    """Both kernels on one operand set -> Results of device tensors."""
    x, ps, pb = wrap(op.x), wrap(op.pscale), wrap(op.pshift)
    pooled, logits = _run_fwd(x, ps, pb, wrap(op.w.t().contiguous()), wrap(op.bias))
    gpooled, gx = _run_bwd(wrap(op.g), wrap(op.w), x, ps, pb)
    return dref.Results(pooled, logits, gpooled, gx)


def _cpu(res):
    return dref.Results(*(t.cpu() for t in res))


@pytest.mark.parametrize("row", dref.ROWS, ids=str)
def test_dense_head_against_the_restatement(row):
    """Forward and input gradient of one row on the exact leg (all four outputs bit for bit) and on the gaussian leg
    (pooled, logits, gpooled within the derived bounds, gx bit for bit from the kernel's own gpooled, the channels with
    pre == 0 included).  Row names and operands are those of tests/test_dense_head_cpu.py, where the emulation passes them."""
    name = dref.row_name(row, "exact")
    op, want = dref.exact_references(name, *row)
    dref.compare_exact(name, _cpu(_run(op)), want)
    name = dref.row_name(row, "gaussian")
    op = dref.operands(name, "gaussian", *row)
    ratios = dref.gaussian_ratios(name, op, _cpu(_run(op)))
    print(name, "max |err| / bound: pooled %.3f logits %.3f gpooled %.3f" % ratios)
    assert max(ratios) <= 1.0, (name, ratios)


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


@pytest.mark.parametrize("row", dref.NAN_ROWS, ids=str)
def test_dense_head_reads_nothing_outside_its_operands(row):
    """x, pscale, pshift, w, wt, bias and g surrounded by NaN, the outputs by canaries: the tails in B, C, HW and N are
    predicated, not read from behind the operand.  The result holds no NaN and equals the plain run and the restatement bit
    for bit; the canaries are intact (`_run_fwd`, `_run_bwd`)."""
    name = dref.row_name(row, "exact")
    op, want = dref.exact_references(name, *row)
    plain, got = _run(op), _run(op, _in_nan)
    for a, b in zip(plain, got):
        assert bool(torch.isfinite(b.float()).all()) and _same_bits(a, b)
    dref.compare_exact(name, _cpu(got), want)


def test_dense_head_refuses_and_leaves_outputs_untouched():
    """Each NULL pointer, each misaligned pointer (x, pscale and gx among them), C = 12, C = 2056, B = 0, HW = 0, N = 0 and
    the sizes just beyond the domain: ADIL_EINVAL, canaries intact; then one accepted call writes exactly the output extents."""
    o, lib = ops(), _lib()
    xin = torch.zeros(1 << 14, dtype=BF16, device=DEV)
    tab = torch.zeros(1 << 14, dtype=F32, device=DEV)
    outf = [torch.full((1 << 12,), CANARY, dtype=F32, device=DEV) for _ in range(3)]
    outx = torch.full((1 << 14,), CANARY, dtype=BF16, device=DEV)
    odd = torch.zeros(64, dtype=torch.uint8, device=DEV)
    P, S = o._ptr, o._stream
    ok = (2, 9, 16, 5)

    def fwd(*a):
        return lib.adil_bn_pool_head_fwd(*a, S())

    def bwd(*a):
        return lib.adil_bn_pool_head_bwd(*a, S())

    fa = (P(xin), P(tab), P(tab), P(tab), P(tab), P(outf[0]), P(outf[1]))       # x pscale pshift wt bias pooled logits
    ba = (P(tab), P(tab), P(xin), P(tab), P(tab), P(outf[2]), P(outx))          # g w x pscale pshift gpooled gx
    sizes = []
    for i, beyond in enumerate((65536, 65537, 2056, 65536)):
        for v in (0, -1, beyond):
            sizes.append(tuple(v if j == i else ok[j] for j in range(4)))
    sizes += [(2, 9, 12, 5), (2, 9, 4, 5)]
    assert all(s in sizes for s in ((0, 9, 16, 5), (2, 0, 16, 5), (2, 9, 16, 0), (2, 9, 2056, 5), (2, 9, 12, 5)))
    for dims in sizes:
        assert fwd(*fa, *dims) == EINVAL, dims
        assert bwd(*ba, *dims) == EINVAL, dims
    for i in range(7):                                                 # each NULL pointer
        assert fwd(*(None if j == i else v for j, v in enumerate(fa)), *ok) == EINVAL, i
        assert bwd(*(None if j == i else v for j, v in enumerate(ba)), *ok) == EINVAL, i
    mis = (P(xin[4:]), P(tab[1:]), P(tab[2:]), P(tab[1:]), P(odd[1:]), P(outf[0][1:]), P(outf[1][2:]))
    for i in range(7):
        assert fwd(*(mis[j] if j == i else v for j, v in enumerate(fa)), *ok) == EINVAL, i
    mis = (P(tab[1:]), P(tab[2:]), P(xin[4:]), P(tab[1:]), P(tab[2:]), P(outf[2][1:]), P(outx[4:]))
    for i in range(7):
        assert bwd(*(mis[j] if j == i else v for j, v in enumerate(ba)), *ok) == EINVAL, i
    torch.cuda.synchronize()
    assert all(bool((t == CANARY).all()) for t in outf) and bool((outx == CANARY).all())
    # accepted: bias on any 4-byte boundary; exactly the output extents are written
    B, HW, C, N = ok
    assert fwd(P(xin), P(tab), P(tab), P(tab), P(tab[1:]), P(outf[0]), P(outf[1]), *ok) == 0
    assert bwd(*ba, *ok) == 0
    torch.cuda.synchronize()
    for t, n in ((outf[0], B * C), (outf[1], B * N), (outf[2], B * C), (outx, B * HW * C)):
        assert bool((t[:n] == 0).all()) and bool((t[n:] == CANARY).all()), n


def test_dense_head_beyond_2_31_elements():
    """B = 513 images of 64 x 64 x 1024: x and gx hold 2^31 + 2^22 elements, the whole last image lies beyond element 2^31
    (the gradient pass reads x there as well as writing gx).  Exact-leg operands built on the device: image b has the integer
    target pre-activation T[b][c] on its even pixels and -T[b][c] on its odd ones, so S = 2048 |T|, pooled = |T| / 2,
    the even pixels keep the gradient where T > 0 and the odd ones where T < 0: the reference is a formula on [B][C] tensors.
    All four outputs bit for bit; the first and the last image also equal the same images run alone."""
    _need(12)
    B, HW, C, N = 513, 4096, 1024, 8
    assert (B - 1) * HW * C >= 2 ** 31
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen, device=DEV).float()
    pscale = (ri(0, 1, C) * 2 - 1) * 2.0 ** ri(-1, 1, C)
    pshift = ri(-4, 4, C)
    T = ri(-4, 4, B, C)
    w, bias, g = ri(-4, 4, N, C), ri(-4, 4, N), ri(-4, 4, B, N)
    xe, xo = ((t - pshift) / pscale for t in (T, -T))
    assert torch.equal(xe.bfloat16().float(), xe) and torch.equal(xo.bfloat16().float(), xo)
    x = torch.empty((B, HW, C), dtype=BF16, device=DEV)
    x[:, 0::2] = xe.bfloat16()[:, None, :]
    x[:, 1::2] = xo.bfloat16()[:, None, :]
    pooled, logits = _run_fwd(x, pscale, pshift, w.t().contiguous(), bias)
    want_pooled = T.abs() / 2
    assert torch.equal(pooled, want_pooled) and bool((pooled != 0).any())
    want_logits = (want_pooled.double() @ w.double().t() + bias.double()).float()      # multiples of 1/2 below 2^23: exact
    assert torch.equal(logits, want_logits)
    gpooled, gx = _run_bwd(g, w, x, pscale, pshift)
    assert torch.equal(gpooled, (g.double() @ w.double()).float())
    v = ((gpooled * dref.href.inv_hw(HW).to(DEV)) * pscale).bfloat16()
    zero = torch.zeros((), dtype=BF16, device=DEV)
    ve, vo = torch.where(T > 0, v, zero), torch.where(T < 0, v, zero)
    assert bool((ve != 0).any()) and bool((vo != 0).any())
    for b0 in range(0, B, 64):
        part = gx[b0:b0 + 64]
        assert bool((part[:, 0::2] == ve[b0:b0 + 64, None, :]).all()) and bool((part[:, 1::2] == vo[b0:b0 + 64, None, :]).all()), b0
    for b in (0, B - 1):
        p1, l1 = _run_fwd(x[b:b + 1], pscale, pshift, w.t().contiguous(), bias)
        q1, x1 = _run_bwd(g[b:b + 1].contiguous(), w, x[b:b + 1], pscale, pshift)
        assert _same_bits(pooled[b:b + 1], p1) and _same_bits(logits[b:b + 1], l1), b
        assert _same_bits(gpooled[b:b + 1], q1) and _same_bits(gx[b:b + 1], x1) and bool((x1 != 0).any()), b


AUTOGRAD_ROWS = [(3, 7, 7, 24, 10), (17, 3, 3, 40, 7), (2, 2, 2, 1024, 1000)]


def _nchw(x3, h, w):
    """[B][HW][C] -> the (B, C, H, W) channels_last tensor with that storage."""
    return x3.reshape(x3.shape[0], h, w, x3.shape[2]).permute(0, 3, 1, 2)


@pytest.mark.parametrize("b,h,w,c,n", AUTOGRAD_ROWS)
def test_autograd_function_equals_the_c_abi_bitwise(b, h, w, c, n):
    """ops.bn_pool_head on the channels_last activation: the very bits of the C-ABI calls, fp32 logits, a bf16 channels_last
    gradient; a bf16 or mis-shaped logit gradient, wrong dtypes, layouts and shapes raise ValueError."""
    o = ops()
    op = dref.operands("autograd/%s" % ((b, h, w, c, n),), "gaussian", b, h * w, c, n)
    want = _run(op)
    ps, pb, wd, wt, bias = _dev(op.pscale), _dev(op.pshift), _dev(op.w), _dev(op.w.t().contiguous()), _dev(op.bias)
    x = _nchw(_dev(op.x), h, w).requires_grad_(True)
    assert o.bn_pool_head_covers(x, c) and not o.bn_pool_head_covers(x, c + 8) and not o.bn_pool_head_covers(x.float(), c)
    logits = o.bn_pool_head(x, ps, pb, wd, wt, bias)
    assert logits.shape == (b, n) and logits.dtype == F32 and logits.is_contiguous()
    assert _same_bits(logits.detach(), want.logits)
    gt = _dev(op.g.t().contiguous()).t()                                # a logit gradient that is not contiguous
    (gx,) = torch.autograd.grad(logits, x, gt, retain_graph=True)
    assert gx.shape == x.shape and gx.dtype == BF16 and gx.is_contiguous(memory_format=torch.channels_last)
    assert _same_bits(gx.permute(0, 2, 3, 1).reshape(b, h * w, c), want.gx)
    with pytest.raises(ValueError):
        o.BnPoolHeadFunction.backward(logits.grad_fn, _dev(op.g).bfloat16())           # a bf16 logit gradient
    with pytest.raises(ValueError):
        o.BnPoolHeadFunction.backward(logits.grad_fn, _dev(op.g)[:, :-1] if n > 1 else _dev(op.g)[:0])   # mis-shaped
    with pytest.raises(ValueError):
        o.bn_pool_head(x.float(), ps, pb, wd, wt, bias)
    with pytest.raises(ValueError):
        o.bn_pool_head(x.detach().contiguous(), ps, pb, wd, wt, bias)                   # NCHW storage
    with pytest.raises(ValueError):
        o.bn_pool_head(x, ps.double(), pb, wd, wt, bias)
    with pytest.raises(ValueError):
        o.bn_pool_head(x, ps, pb[:-1], wd, wt, bias)
    with pytest.raises(ValueError):
        o.bn_pool_head(x, ps, pb, wd, wd, bias)                                         # wt not transposed


def test_dense_head_in_a_captured_graph():
    """Forward + input gradient captured in a graph on a single stream (four launches in a chain, no parallel branch) and
    replayed on fresh operand contents copied into the captured buffers equals the eager result bit for bit."""
    o = ops()
    b, h, w, c, n = 4, 7, 7, 1024, 1000
    op = dref.operands("graph", "gaussian", b, h * w, c, n)
    op2 = dref.operands("graph/2", "gaussian", b, h * w, c, n)
    args = [_dev(t).clone() for t in (op.pscale, op.pshift, op.w, op.w.t().contiguous(), op.bias)]

    def run(x, g, a):
        logits = o.bn_pool_head(x, *a)
        (gx,) = torch.autograd.grad(logits, x, g)
        return logits, gx

    def args_of(q):
        return [_dev(t) for t in (q.pscale, q.pshift, q.w, q.w.t().contiguous(), q.bias)]

    eager = [tuple(t.detach().clone() for t in run(_nchw(_dev(q.x), h, w).requires_grad_(True), _dev(q.g), args_of(q)))
             for q in (op, op2)]
    xs = _nchw(_dev(op.x).clone(), h, w).requires_grad_(True)
    gs = _dev(op.g).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(xs, gs, args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ls, gxs = run(xs, gs, args)
    for q, (want_l, want_gx) in zip((op2, op), eager[::-1]):
        with torch.no_grad():
            xs.copy_(_nchw(_dev(q.x), h, w))
            gs.copy_(_dev(q.g))
            for dst, src in zip(args, args_of(q)):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(ls.detach(), want_l)
        assert _same_bits(gxs.permute(0, 2, 3, 1), want_gx.permute(0, 2, 3, 1))


# ------------------------------------------------------------------------------------------------------------- network
def randomised_checkpoint(path, seed=5, num_classes=1000):
    """The recipe of tests/test_gpu_dense_transition.randomised_checkpoint, restated: a seeded DenseNet-121 state_dict with
    BatchNorm statistics drawn around the initial 0 / 1 and gamma of BOTH signs."""
    from dl_attack_on_imagenet_amd import zoo
    model = zoo.build_classifier("densenet121", num_classes=num_classes, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    r = lambda n: torch.randn(n, generator=gen)
    u = lambda n: torch.rand(n, generator=gen)
    sign = lambda n: (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_((0.7 + 0.6 * u(n)) * sign(n))
                m.bias.copy_(0.2 * r(n))
                m.running_mean.copy_(0.2 * r(n))
                m.running_var.copy_(0.6 + 0.8 * u(n))
    torch.save(model[1].state_dict(), path)
    return path


def _forward_and_gradient(model, x):
    x = x.clone().requires_grad_(True)
    out = model(x)
    logits = out.float()
    (g,) = torch.autograd.grad(logits.square().sum(), x)
    return out.dtype, logits.detach(), g.detach().float()


COUNTED = ((F, "conv2d"), (F, "avg_pool2d"), (F, "max_pool2d"), (torch, "cat"), (F, "batch_norm"), (F, "adaptive_avg_pool2d"),
           (F, "linear"), (F, "relu"))


def _library_calls(monkeypatch, model, x):
    """How often one forward of `model` calls each of COUNTED."""
    counts = OrderedDict()
    with monkeypatch.context() as mp:
        for owner, name in COUNTED:
            counts[name] = []
            mp.setattr(owner, name, lambda *a, _real=getattr(owner, name), _c=counts[name], **k: (_c.append(1), _real(*a, **k))[1])
        with torch.no_grad():
            model(x)
    return {k: len(v) for k, v in counts.items()}


def test_densenet_on_all_six_dense_switches(tmp_path, monkeypatch):
    """All six dense switches, and `own_dense_head=True` alone, on 4 structured images at 64 x 64 and a 1000-class checkpoint
    with randomised BatchNorm statistics: fp32 logits against the fp32 network within the bf16 depth bound of 121 layers, the
    input gradient no further from the fp32 network's than 1.5 x the distance of the plain bf16 network; the head's kernel
    output on its ACTUAL input under the gaussian-leg bounds (restated in a forward hook); with all six switches no library
    call is left (F.conv2d, F.avg_pool2d, F.max_pool2d, torch.cat, F.batch_norm, F.adaptive_avg_pool2d, F.linear 0 times
    each, F.relu once less than with five switches); with the head alone F.batch_norm, F.adaptive_avg_pool2d and F.linear
    lose exactly one call each; two fresh builds give bitwise equal logits and input gradients."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import zoo
    images, _ = structured_images(4, classes=4, seed=3, size=64)
    path = randomised_checkpoint(os.path.join(str(tmp_path), "densenet_random_bn.pt"))
    kw = dict(num_classes=1000, seed=5, weights=path, device=DEV)
    x = images.to(DEV)
    _, lr, gr = _forward_and_gradient(zoo.build_classifier("densenet121", **kw), x)
    kw.update(dtype=BF16, channels_last=True)
    plain = zoo.build_classifier("densenet121", **kw)
    d0, l0, g0 = _forward_and_gradient(plain, x.bfloat16())
    rms = float(lr.square().mean().sqrt())
    bound = _bf16_depth_bound(121) * rms
    rel = lambda g: float((g - gr).norm() / gr.norm())
    e0, r0 = float((l0 - lr).abs().mean()), rel(g0)
    assert float(gr.abs().max()) > 0 and d0 == BF16
    five = zoo.build_classifier("densenet121", **FIVE, **kw)
    six = zoo.build_classifier("densenet121", own_dense_head=True, **FIVE, **kw)
    alone = zoo.build_classifier("densenet121", own_dense_head=True, **kw)
    head = six[0].head32
    assert isinstance(head, zoo._OwnDenseHead) and six[0].head32_on and head.weight.dtype == F32 and head.pscale.dtype == F32
    assert six[0].classifier.weight.dtype == BF16 and bool((head.pscale < 0).any())
    seen = []

    def restate(mod, args, out):
        xin = args[0].detach()
        assert xin.dtype == BF16 and tuple(xin.shape[1:]) == (1024, 2, 2) and xin.is_contiguous(memory_format=torch.channels_last)
        x3 = xin.permute(0, 2, 3, 1).reshape(xin.shape[0], 4, 1024)
        pooled, logits = _run_fwd(x3, mod.pscale, mod.pshift, mod.wt, mod.bias)
        assert _same_bits(logits, out.detach())
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
        gpooled, gx = _run_bwd(g, mod.weight, x3, mod.pscale, mod.pshift)
        op = dref.Operands(x3.cpu(), mod.pscale.cpu(), mod.pshift.cpu(), mod.weight.cpu(), mod.bias.cpu(), g.cpu(), None)
        masked = float((~(dref.pre_of(dref.Arith(), op.x, op.pscale, op.pshift) > 0)).double().mean())
        seen.append(dref.gaussian_ratios("net/head", op, dref.Results(pooled.cpu(), logits.cpu(), gpooled.cpu(), gx.cpu())) + (masked,))

    handle = head.register_forward_hook(restate)
    d6, l6, g6 = _forward_and_gradient(six, x.bfloat16())
    handle.remove()
    d1, l1, g1 = _forward_and_gradient(alone, x.bfloat16())
    assert d6 == F32 and d1 == F32 and len(seen) == 1
    print("head 1024 -> 1000 at 2 x 2 on its real input: max |err| / bound pooled %.3f logits %.3f gpooled %.3f; masked %.2f" % seen[0])
    assert max(seen[0][:3]) <= 1.0 and 0.0 < seen[0][3] < 1.0, seen
    e6, e1 = (float((l - lr).abs().mean()) for l in (l6, l1))
    r6, r1 = rel(g6), rel(g1)
    print("logit error vs fp32: plain bf16 %.5f six switches %.5f head alone %.5f, rms %.4f, bound %.5f; input gradient relative "
          "error vs fp32: plain bf16 %.4f six switches %.4f head alone %.4f" % (e0, e6, e1, rms, bound, r0, r6, r1))
    for l, g in ((l6, g6), (l1, g1)):
        assert torch.isfinite(l).all() and torch.isfinite(g).all() and g.shape == x.shape and float(g.abs().max()) > 0
    assert max(e6, e1) <= bound, (e0, e6, e1, rms)
    assert max(r6, r1) <= 1.5 * r0, (r0, r6, r1)
    n0, n5, n6, n1 = (_library_calls(monkeypatch, m, x.bfloat16()) for m in (plain, five, six, alone))
    print("library calls per forward: plain %s\nfive switches %s\nsix switches %s\nhead alone %s" % (n0, n5, n6, n1))
    assert n5["batch_norm"] == 1 and n5["adaptive_avg_pool2d"] == 1 and n5["linear"] == 1
    for name in ("conv2d", "avg_pool2d", "max_pool2d", "cat", "batch_norm", "adaptive_avg_pool2d", "linear"):
        assert n6[name] == 0, (name, n6)
    assert n6["relu"] == n5["relu"] - 1, (n5, n6)
    for name in ("batch_norm", "adaptive_avg_pool2d", "linear"):
        assert n1[name] == n0[name] - 1, (name, n0, n1)
    for name in ("conv2d", "avg_pool2d", "max_pool2d", "cat"):
        assert n1[name] == n0[name], (name, n0, n1)
    again = zoo.build_classifier("densenet121", own_dense_head=True, **FIVE, **kw)
    _, l7, g7 = _forward_and_gradient(again, x.bfloat16())
    assert torch.equal(l6, l7) and torch.equal(g6, g7)


def test_inference_mode_enters_the_dense_head_in_the_solver_only(monkeypatch):
    """own_dense_head="inference" at 64 x 64, 10 classes, all six switches: a plain call and the learner's step keep bf16
    logits and never call ops.bn_pool_head, the DDrague solver calls it once per iteration, and the two heads agree to one
    bf16 rounding of the fp32 logits."""
    from dl_attack_on_imagenet_amd import engine, zoo
    o = ops()
    net = zoo.build_classifier("densenet121", num_classes=10, seed=3, device=DEV, dtype=BF16, channels_last=True,
                               own_dense_head="inference", **FIVE)
    dense = net[0]
    assert isinstance(dense.head32, zoo._OwnDenseHead) and not dense.head32_on
    calls, real = {"n": 0}, o.bn_pool_head
    monkeypatch.setattr(o, "bn_pool_head", lambda *a: (calls.__setitem__("n", calls["n"] + 1), real(*a))[1])
    g = torch.Generator().manual_seed(12)
    x = torch.rand(8, 3, 64, 64, generator=g).to(DEV).to(BF16)
    plain = net(x)
    assert plain.dtype == BF16 and calls["n"] == 0
    with engine.precise_head(net):
        sharp = net(x)
    assert sharp.dtype == F32 and calls["n"] == 1 and not dense.head32_on
    diff, top = float((sharp - plain.float()).abs().max()), float(sharp.abs().max())
    print("fp32 head against the library bf16 head: max |difference| %.5f, max |logit| %.4f" % (diff, top))
    assert diff <= 2.0 ** -7 * top + 1e-3                                # one bf16 rounding of the logits
    d = (-1 + 2 * torch.rand(3, 64, 64, 6, generator=g)).to(DEV)
    v = o.l1ball_project_(torch.rand(8, 6, generator=g).to(DEV), 0.1)
    learner = engine.DictionaryLearner(d.clone(), v, 0.1, 0.01, "logits")
    learner.step(net, x, torch.arange(8, device=DEV))
    assert calls["n"] == 1                                              # the learner keeps the library head
    engine.DDragueSolver(net, x, d, 0.1, "logits").run(9)
    assert calls["n"] == 1 + 9 and not dense.head32_on                   # once per inference iteration


def test_dense_head_is_bitwise_across_processes():
    """One fresh child process under `timeout` prints the digests of the logits and the input gradient of the six-switch
    network; they equal the digests this process computes."""
    import dense_head_child
    child = os.path.join(ROOT, "tests", "dense_head_child.py")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, child], env=env, capture_output=True, text=True,
                       timeout=270, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("hash ")]
    assert len(lines) == 2, r.stdout[-2000:]
    assert lines == dense_head_child.network_digests()
