"""GPU: the pooled fp32 head kernels (adil_pool_head_fwd / adil_pool_head_bwd, csrc/adil_head.hip) through the C ABI against
the fp64 restatement of tests/head_reference.py — bit for bit on the exact leg, under the derived elementwise bounds on the
gaussian leg — and the MobileNetV2 that runs its pooling and classifier on them (`head_fp32=True | "inference"`), alone and
with `own_depthwise`, `own_pointwise` and `own_first_conv`, when no library call is left in the network."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import head_reference as href
from classifier_reference import BF16, CANARY, F32
from graph_tools import assert_graph_used, no_capture_fallback

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PAD = 256                        # canary elements in front of and behind every output


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


def _run_fwd(x, wt, bias):
    """Device tensors in (x [B][HW][C] bf16, wt [C][N], bias [N]); pooled [B][C] and logits [B][N] out, canaries around both."""
    o, lib = ops(), _lib()
    B, HW, C = x.shape
    N = wt.shape[1]
    pbuf, pooled = _guarded((B, C), F32)
    lbuf, logits = _guarded((B, N), F32)
    assert lib.adil_pool_head_fwd(o._ptr(x), o._ptr(wt), o._ptr(bias), o._ptr(pooled), o._ptr(logits), B, HW, C, N,
                                  o._stream()) == 0
    torch.cuda.synchronize()
    assert _intact(pbuf) and _intact(lbuf), "forward wrote outside pooled / logits"
    return pooled, logits


def _run_bwd(g, w, HW):
    o, lib = ops(), _lib()
    B, N = g.shape
    C = w.shape[1]
    pbuf, gpooled = _guarded((B, C), F32)
    xbuf, gx = _guarded((B, HW, C), BF16)
    assert lib.adil_pool_head_bwd(o._ptr(g), o._ptr(w), o._ptr(gpooled), o._ptr(gx), B, HW, C, N, o._stream()) == 0
    torch.cuda.synchronize()
    assert _intact(pbuf) and _intact(xbuf), "gradient wrote outside gpooled / gx"
    return gpooled, gx


def _run(op, wrap=_dev):
    """Both kernels on one operand set -> head_reference.Results of device tensors."""
    pooled, logits = _run_fwd(wrap(op.x), wrap(op.w.t().contiguous()), wrap(op.bias))
    gpooled, gx = _run_bwd(wrap(op.g), wrap(op.w), op.x.shape[1])
    return href.Results(pooled, logits, gpooled, gx)


def _cpu(res):
    return href.Results(*(t.cpu() for t in res))


@pytest.mark.parametrize("row", href.ROWS, ids=str)
def test_head_against_the_fp64_restatement(row):
    """Forward and input gradient of one row on the exact leg (all four outputs bit for bit) and on the gaussian leg
    (pooled, logits, gpooled within the derived bounds, gx bit for bit from the kernel's own gpooled).  Row names and
    operands are those of tests/test_head_cpu.py, where the emulation passes them."""
    name = href.row_name(row, "exact")
    op, want = href.exact_references(name, *row)
    href.compare_exact(name, _cpu(_run(op)), want)
    name = href.row_name(row, "gaussian")
    op = href.operands(name, "gaussian", *row)
    ratios = href.gaussian_ratios(name, op, _cpu(_run(op)))
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


@pytest.mark.parametrize("row", href.NAN_ROWS, ids=str)
def test_head_reads_nothing_outside_its_operands(row):
    """x, w, wt, bias and g surrounded by NaN, the outputs by canaries: the tails in B, C, HW and N are predicated, not read
    from behind the operand.  The result holds no NaN and equals the plain run and the restatement bit for bit."""
    name = href.row_name(row, "exact")
    op, want = href.exact_references(name, *row)
    plain, got = _run(op), _run(op, _in_nan)
    for a, b in zip(plain, got):
        assert bool(torch.isfinite(b.float()).all()) and _same_bits(a, b)
    href.compare_exact(name, _cpu(got), want)


def test_head_refuses_and_leaves_outputs_untouched():
    """Each NULL pointer, each size at 0, -1 and just beyond the domain, C = 12, misaligned pointers: ADIL_EINVAL, canaries
    intact; then one accepted call writes exactly the output extents."""
    o, lib = ops(), _lib()
    xin = torch.zeros(1 << 14, dtype=BF16, device=DEV)
    tab = torch.zeros(1 << 14, dtype=F32, device=DEV)
    outf = [torch.full((1 << 12,), CANARY, dtype=F32, device=DEV) for _ in range(3)]
    outx = torch.full((1 << 14,), CANARY, dtype=BF16, device=DEV)
    odd = torch.zeros(64, dtype=torch.uint8, device=DEV)
    P, S = o._ptr, o._stream
    ok = (2, 9, 16, 5)

    def fwd(x, wt, bias, pooled, logits, B, HW, C, N):
        return lib.adil_pool_head_fwd(x, wt, bias, pooled, logits, B, HW, C, N, S())

    def bwd(g, w, gpooled, gx, B, HW, C, N):
        return lib.adil_pool_head_bwd(g, w, gpooled, gx, B, HW, C, N, S())

    fa = (P(xin), P(tab), P(tab), P(outf[0]), P(outf[1]))
    ba = (P(tab), P(tab), P(outf[2]), P(outx))
    sizes = []
    for i, beyond in enumerate((65536, 65537, 2056, 65536)):
        for v in (0, -1, beyond):
            sizes.append(tuple(v if j == i else ok[j] for j in range(4)))
    sizes += [(2, 9, 12, 5), (2, 9, 4, 5), (2, 9, 0, 5)]
    for dims in sizes:
        assert fwd(*fa, *dims) == EINVAL, dims
        assert bwd(*ba, *dims) == EINVAL, dims
    for i in range(5):                                                 # each NULL pointer of the forward
        assert fwd(*(None if j == i else v for j, v in enumerate(fa)), *ok) == EINVAL, i
    for i in range(4):                                                 # and of the gradient
        assert bwd(*(None if j == i else v for j, v in enumerate(ba)), *ok) == EINVAL, i
    mis = (P(xin[4:]), P(tab[1:]), P(odd[1:]), P(outf[0][1:]), P(outf[1][2:]))     # 8, 4, 1, 4, 8 bytes off
    for i in range(5):
        assert fwd(*(mis[j] if j == i else v for j, v in enumerate(fa)), *ok) == EINVAL, i
    mis = (P(tab[1:]), P(tab[2:]), P(outf[2][1:]), P(outx[4:]))
    for i in range(4):
        assert bwd(*(mis[j] if j == i else v for j, v in enumerate(ba)), *ok) == EINVAL, i
    torch.cuda.synchronize()
    assert all(bool((t == CANARY).all()) for t in outf) and bool((outx == CANARY).all())
    # accepted: bias on any 4-byte boundary; exactly the output extents are written
    B, HW, C, N = ok
    assert fwd(P(xin), P(tab), P(tab[1:]), P(outf[0]), P(outf[1]), *ok) == 0
    assert bwd(*ba, *ok) == 0
    torch.cuda.synchronize()
    for t, n in ((outf[0], B * C), (outf[1], B * N), (outf[2], B * C), (outx, B * HW * C)):
        assert bool((t[:n] == 0).all()) and bool((t[n:] == CANARY).all()), n


def test_head_beyond_2_31_elements():
    """B = 536 images of 56 x 56 x 1280: x and gx hold 2.15e9 elements, so the whole last image lies beyond element 2^31.
    The first and the last image equal the same images run alone, bit for bit, both ways; image 0 carries the operands of
    the exact leg and is compared with the restatement."""
    _need(12)
    B, HW, C, N = 536, 3136, 1280, 8
    assert (B - 1) * HW * C > 2 ** 31
    op, want = href.exact_references("big", 1, HW, C, N)
    w, wt, bias = _dev(op.w), _dev(op.w.t().contiguous()), _dev(op.bias)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    x = torch.empty((B, HW, C), dtype=BF16, device=DEV)
    for b0 in range(0, B, 64):
        part = x[b0:b0 + 64]
        part.copy_(torch.randint(-4, 5, part.shape, generator=gen, device=DEV, dtype=torch.int8))
    x[0].copy_(op.x[0])
    g = torch.randint(-4, 5, (B, N), generator=gen, device=DEV).float()
    g[0].copy_(op.g[0])
    pooled, logits = _run_fwd(x, wt, bias)
    for b in (0, B - 1):
        p1, l1 = _run_fwd(x[b:b + 1], wt, bias)
        assert _same_bits(pooled[b:b + 1], p1) and _same_bits(logits[b:b + 1], l1) and bool((p1 != 0).any()), b
    del x
    gpooled, gx = _run_bwd(g, w, HW)
    for b in (0, B - 1):
        q1, x1 = _run_bwd(g[b:b + 1].contiguous(), w, HW)
        assert _same_bits(gpooled[b:b + 1], q1) and _same_bits(gx[b:b + 1], x1) and bool((x1 != 0).any()), b
    href.compare_exact("big/0", href.Results(pooled[:1].cpu(), logits[:1].cpu(), gpooled[:1].cpu(), gx[:1].cpu()), want)


AUTOGRAD_ROWS = [(3, 7, 7, 24, 10), (17, 3, 3, 40, 7), (2, 4, 4, 1280, 1000)]


def _nchw(x3, h, w):
    """[B][HW][C] -> the (B, C, H, W) channels_last tensor with that storage."""
    return x3.reshape(x3.shape[0], h, w, x3.shape[2]).permute(0, 3, 1, 2)


@pytest.mark.parametrize("b,h,w,c,n", AUTOGRAD_ROWS)
def test_autograd_function_equals_the_c_abi_bitwise(b, h, w, c, n):
    """ops.pool_head on the channels_last activation: no copy in, the very bits of the C-ABI calls, fp32 logits, a bf16
    channels_last gradient; B = 0 launches nothing; wrong dtypes, layouts and shapes raise ValueError."""
    o = ops()
    op = href.operands("autograd/%s" % ((b, h, w, c, n),), "gaussian", b, h * w, c, n)
    want = _run(op)
    wd, wt, bias = _dev(op.w), _dev(op.w.t().contiguous()), _dev(op.bias)
    x = _nchw(_dev(op.x), h, w).requires_grad_(True)
    assert o.pool_head_covers(x, c) and not o.pool_head_covers(x, c + 8) and not o.pool_head_covers(x.float(), c)
    logits = o.pool_head(x, wd, wt, bias)
    assert logits.shape == (b, n) and logits.dtype == F32 and logits.is_contiguous()
    assert _same_bits(logits.detach(), want.logits)
    gt = _dev(op.g.t().contiguous()).t()                                # a logit gradient that is not contiguous
    assert not gt.is_contiguous() or min(b, n) == 1
    (gx,) = torch.autograd.grad(logits, x, gt)
    assert gx.shape == x.shape and gx.dtype == BF16 and gx.is_contiguous(memory_format=torch.channels_last)
    assert _same_bits(gx.permute(0, 2, 3, 1).reshape(b, h * w, c), want.gx)
    x0 = x[:0].detach().requires_grad_(True)
    empty = o.pool_head(x0, wd, wt, bias)                                              # B = 0 launches nothing
    assert empty.shape == (0, n) and empty.dtype == F32
    (ge,) = torch.autograd.grad(empty, x0, torch.zeros(0, n, device=DEV))
    assert ge.shape == (0, c, h, w) and ge.dtype == BF16
    with pytest.raises(ValueError):
        o.pool_head(x.float(), wd, wt, bias)
    with pytest.raises(ValueError):
        o.pool_head(x.detach().contiguous(), wd, wt, bias)                             # NCHW storage
    with pytest.raises(ValueError):
        o.pool_head(x, wd.double(), wt, bias)
    with pytest.raises(ValueError):
        o.pool_head(x, wd, wd, bias)                                                    # wt not transposed
    with pytest.raises(ValueError):
        o.pool_head(x, wd, wt, bias[:-1] if n > 1 else bias.double())
    with pytest.raises(ValueError):
        o.pool_head(x, wd[:, :-8].contiguous(), wt[:-8].contiguous(), bias)            # another channel count


def test_head_in_a_captured_graph():
    """Forward + input gradient captured in a graph on a single stream and replayed (on fresh inputs copied into the
    captured buffers) equals the eager result bit for bit: the calls launch on the capturing stream and neither synchronise
    nor allocate outside the allocator."""
    o = ops()
    b, h, w, c, n = 4, 7, 7, 1280, 1000
    op = href.operands("graph", "gaussian", b, h * w, c, n)
    op2 = href.operands("graph/2", "gaussian", b, h * w, c, n)
    args = (_dev(op.w), _dev(op.w.t().contiguous()), _dev(op.bias))

    def run(x, g):
        logits = o.pool_head(x, *args)
        (gx,) = torch.autograd.grad(logits, x, g)
        return logits, gx

    eager = [tuple(t.detach().clone() for t in run(_nchw(_dev(q.x), h, w).requires_grad_(True), _dev(q.g))) for q in (op, op2)]
    xs = _nchw(_dev(op.x).clone(), h, w).requires_grad_(True)
    gs = _dev(op.g).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(xs, gs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ls, gxs = run(xs, gs)
    for q, (want_l, want_gx) in zip((op, op2), eager):
        with torch.no_grad():
            xs.copy_(_nchw(_dev(q.x), h, w))
            gs.copy_(_dev(q.g))
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(ls.detach(), want_l)
        assert _same_bits(gxs.permute(0, 2, 3, 1), want_gx.permute(0, 2, 3, 1))


# ------------------------------------------------------------------------------------------------------------- network
def randomised_checkpoint(path, seed=5, num_classes=1000):
    """The recipe of tests/test_gpu_first_conv.py (images None), restated: a seeded MobileNetV2 state_dict with randomised
    BatchNorm statistics and affine maps drawn around the initial 0 / 1 (mean 0.2 N(0,1), var in [0.6, 1.4], gamma in
    [0.7, 1.3], beta 0.2 N(0,1)): the network of the precision comparisons."""
    from dl_attack_on_imagenet_amd import zoo
    model = zoo.build_classifier("mobilenet", num_classes=num_classes, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    r = lambda n: torch.randn(n, generator=gen)
    u = lambda n: torch.rand(n, generator=gen)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_(0.7 + 0.6 * u(n))
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
    assert g.shape == x.shape and g.dtype == x.dtype
    return out.dtype, logits.detach(), g.detach().float()


class _Calls:
    """Counts the library calls of a pass: F.linear, F.adaptive_avg_pool2d, F.conv2d, F.batch_norm."""
    NAMES = ("linear", "adaptive_avg_pool2d", "conv2d", "batch_norm")

    def __init__(self, monkeypatch):
        self.n = dict.fromkeys(self.NAMES, 0)
        for name in self.NAMES:
            monkeypatch.setattr(F, name, self._counting(name, getattr(F, name)))

    def _counting(self, name, real):
        def call(*args, **kw):
            self.n[name] += 1
            return real(*args, **kw)
        return call

    def take(self):
        out = tuple(self.n[name] for name in self.NAMES)
        self.n = dict.fromkeys(self.NAMES, 0)
        return out


def test_mobilenet_on_the_own_head(tmp_path, monkeypatch):
    """`head_fp32=True` on 8 structured images at 224 x 224, a checkpoint with randomised BatchNorm statistics: the head's
    kernel output on its real input within the gaussian bounds (restated in a forward hook), the library calls that are left
    (F.linear / F.adaptive_avg_pool2d 1 / 1 without the head, 0 / 0 with it; no convolution and no BatchNorm with all four
    switches), fp32 logits within the bf16 depth bound of 53 layers of the fp32 network (the head adds no bf16 rounding), the
    input gradient no further from the fp32 network's than 1.5 x the distance of the three-switch network."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import zoo
    images, _ = structured_images(8, classes=4, seed=3, size=224)
    path = randomised_checkpoint(os.path.join(str(tmp_path), "mobilenet_random_bn.pt"))
    kw = dict(num_classes=1000, seed=5, weights=path, device=DEV)
    ref = zoo.build_classifier("mobilenet", **kw)
    kw.update(dtype=BF16, channels_last=True)
    own = dict(own_first_conv=True, own_pointwise=True, own_depthwise=True)
    all3 = zoo.build_classifier("mobilenet", **own, **kw)
    all4 = zoo.build_classifier("mobilenet", head_fp32=True, **own, **kw)
    alone = zoo.build_classifier("mobilenet", head_fp32=True, **kw)
    x = images.to(DEV)
    seen = []

    def restate(mod, args, out):
        xin = args[0].detach()
        assert xin.dtype == BF16 and tuple(xin.shape[1:]) == (1280, 7, 7) and xin.is_contiguous(memory_format=torch.channels_last)
        x3 = xin.permute(0, 2, 3, 1).reshape(xin.shape[0], 49, 1280)
        pooled, logits = _run_fwd(x3, mod.wt, mod.bias)
        assert _same_bits(logits, out.detach())
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
        gpooled, gx = _run_bwd(g, mod.weight, 49)
        op = href.Operands(x3.cpu(), mod.weight.cpu(), mod.bias.cpu(), g.cpu(), None)
        seen.append(href.gaussian_ratios("net/head", op, href.Results(pooled.cpu(), logits.cpu(), gpooled.cpu(), gx.cpu())))

    head = all4[0].head32
    assert isinstance(head, zoo._OwnHead) and head.weight.dtype == F32 and all4[0].classifier[-1].weight.dtype == BF16
    handle = head.register_forward_hook(restate)
    calls = _Calls(monkeypatch)
    d4, l4, g4 = _forward_and_gradient(all4, x.bfloat16())
    n4 = calls.take()
    handle.remove()
    d3, l3, g3 = _forward_and_gradient(all3, x.bfloat16())
    n3 = calls.take()
    d1, l1, g1 = _forward_and_gradient(alone, x.bfloat16())
    n1 = calls.take()
    monkeypatch.undo()
    print("library calls (linear, adaptive_avg_pool2d, conv2d, batch_norm): three switches %s, + head %s, head alone %s" % (n3, n4, n1))
    assert n3 == (1, 1, 0, 0) and n4 == (0, 0, 0, 0) and n1 == (0, 0, 52, 52)
    assert d3 == BF16 and d4 == F32 and d1 == F32
    assert len(seen) == 1
    print("head 1280 -> 1000 at 7 x 7 on its real input: max |err| / bound pooled %.3f logits %.3f gpooled %.3f" % seen[0])
    assert max(seen[0]) <= 1.0, seen
    _, lr, gr = _forward_and_gradient(ref, x)
    rms = float(lr.square().mean().sqrt())
    bound = _bf16_depth_bound(53) * rms
    rel = lambda g: float((g - gr).norm() / gr.norm())
    e3, e4, e1 = (float((l - lr).abs().mean()) for l in (l3, l4, l1))
    r3, r4, r1 = rel(g3), rel(g4), rel(g1)
    print("logit error vs fp32: three switches %.5f + head %.5f head alone %.5f, rms %.4f, bound %.5f; input gradient relative "
          "error vs fp32: three switches %.4f + head %.4f head alone %.4f" % (e3, e4, e1, rms, bound, r3, r4, r1))
    assert float(gr.abs().max()) > 0
    for l, g in ((l4, g4), (l1, g1)):
        assert torch.isfinite(l).all() and torch.isfinite(g).all() and g.shape == x.shape and float(g.abs().max()) > 0
    assert max(e4, e1) <= bound, (e3, e4, e1, rms)
    assert max(r4, r1) <= 1.5 * r3, (r3, r4, r1)


def test_inference_mode_enters_the_own_head_in_the_solver_only(monkeypatch):
    """head_fp32="inference" at 64 x 64, 10 classes, all switches: a plain call and the learner's step keep bf16 logits and
    never call the own head, the DDrague solver calls it once per iteration, engine.precise_head nests and restores, and
    the two heads agree to one bf16 rounding of the logits.  With head_fp32=True no library call is left in the
    classifier and a graphed DDrague loop returns the eager loop's adversarial images bit for bit."""
    from dl_attack_on_imagenet_amd import engine, zoo
    o = ops()
    kw = dict(num_classes=10, seed=3, device=DEV, dtype=BF16, channels_last=True, own_depthwise=True, own_pointwise=True,
              own_first_conv=True)
    net = zoo.build_classifier("mobilenet", head_fp32="inference", **kw)
    mob = net[0]
    assert isinstance(mob.head32, zoo._OwnHead) and mob.head32.weight.dtype == F32 and not mob.head32_on
    calls = {"n": 0}
    mob.head32.register_forward_hook(lambda *a: calls.__setitem__("n", calls["n"] + 1))
    g = torch.Generator().manual_seed(12)
    x = torch.rand(8, 3, 64, 64, generator=g).to(DEV).to(BF16)
    plain = net(x)
    assert plain.dtype == BF16 and calls["n"] == 0
    with engine.precise_head(net):
        sharp = net(x)
        with engine.precise_head(net, False):                      # nests and restores
            assert net(x).dtype == BF16
        assert mob.head32_on
    assert sharp.dtype == F32 and calls["n"] == 1 and not mob.head32_on
    assert float((sharp - plain.float()).abs().max()) <= 2.0 ** -7 * float(sharp.abs().max()) + 1e-3   # one bf16 rounding of the logits
    d = (-1 + 2 * torch.rand(3, 64, 64, 6, generator=g)).to(DEV)
    v = o.l1ball_project_(torch.rand(8, 6, generator=g).to(DEV), 0.1)
    learner = engine.DictionaryLearner(d.clone(), v, 0.1, 0.01, "logits")
    before = calls["n"]
    learner.step(net, x, torch.arange(8, device=DEV))
    assert calls["n"] == before                                     # the learner keeps the bf16 head
    engine.DDragueSolver(net, x, d, 0.1, "logits").run(9)
    assert calls["n"] == before + 9 and not mob.head32_on           # once per inference iteration
    always = zoo.build_classifier("mobilenet", head_fp32=True, **kw)
    counted = _Calls(monkeypatch)
    assert always(x).dtype == F32
    left = counted.take()
    monkeypatch.undo()
    assert left == (0, 0, 0, 0), left                               # no library call is left in the classifier
    eager = engine.DDragueSolver(always, x, d, 0.1, "logits").run(9)
    with no_capture_fallback():                                     # a failed capture is an error, not an eager run
        graphed = engine.DDragueSolver(always, x, d, 0.1, "logits").run(9, use_graph=True)
    assert_graph_used(graphed)
    adv_e, adv_g = eager.result()[0], graphed.result()[0]
    assert graphed.iters == 9 and bool(torch.isfinite(adv_e.float()).all()) and bool((adv_e != x).any())
    assert _same_bits(adv_e, adv_g)


def test_head_is_bitwise_across_processes():
    """Two fresh child processes, one after the other (the second only if the first exited 0), each under `timeout`:
    byte-identical pooled, logits, gpooled and gx for three rows, and byte-identical logits and input gradient of the
    all-switches MobileNetV2."""
    child = os.path.join(ROOT, "tests", "head_child.py")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
    outs = []
    for _ in range(2):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, child], env=env, capture_output=True, text=True,
                           timeout=270, cwd=ROOT)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("hash ")]
        assert len(lines) == 14, r.stdout[-2000:]              # three rows x four outputs, logits and gradient of the network
        outs.append(lines)
    for a, b in zip(*outs):
        assert a == b, (a, b)
