"""GPU: the pool-first transition kernels (adil_dense_transition_fwd / adil_dense_transition_bwd,
csrc/adil_dense_transition.hip) through the C ABI against the fp64 restatement of tests/dense_transition_reference.py —
bit for bit on the exact legs, under the derived elementwise bound on the gaussian leg — the strided gradient operand, the
autograd function, a captured graph, the stem wiring of `own_dense_stem`, and the DenseNet-121 with all five dense
switches on."""
import os
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

import dense1x1_reference as d1
import dense_transition_reference as tr
from classifier_reference import BF16, CANARY, Arith

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
EINVAL = -1
PAD = 5                          # canary rows behind every output
NAN = float("nan")
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def ops():
    from dl_attack_on_imagenet_amd import ops as o
    return o


def _lib():
    return __import__("dl_attack_on_imagenet_amd._lib", fromlist=["x"]).load()


def _dev(t):
    return t.to(DEV).contiguous()


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _bf16_depth_bound(layers: int) -> float:
    """The bound of tests/test_gpu_stem.py, restated: mean |logit error| of a bf16-activation network against its fp32
    twin relative to the rms logit; `layers` roundings of relative size 2^-9 in series add in quadrature, times 2 for a
    relative gain above 1 in a random-weight network."""
    return 2.0 * 2.0 ** -9 * layers ** 0.5


def _run_fwd(dims, x, pscale, pshift, w):
    """Device tensors in, y [Mo][N] out; canary rows behind y."""
    o, lib = ops(), _lib()
    B, H, W, K, N = dims
    Mo = B * (H // 2) * (W // 2)
    y = torch.full((Mo + PAD, N), CANARY, dtype=BF16, device=DEV)
    assert lib.adil_dense_transition_fwd(o._ptr(x), o._ptr(pscale), o._ptr(pshift), o._ptr(w), o._ptr(y), B, H, W, K, N,
                                         o._stream()) == 0
    torch.cuda.synchronize()
    assert bool((y[Mo:] == CANARY).all()), "forward wrote past the end of y"
    return y[:Mo]


def _run_bwd(dims, g, ldg, wt, xin, pscale, pshift):
    o, lib = ops(), _lib()
    B, H, W, K, N = dims
    Min = B * H * W
    gx = torch.full((Min + PAD, K), CANARY, dtype=BF16, device=DEV)
    assert lib.adil_dense_transition_bwd(o._ptr(g), ldg, o._ptr(wt), o._ptr(xin), o._ptr(pscale), o._ptr(pshift), o._ptr(gx),
                                         B, H, W, K, N, o._stream()) == 0
    torch.cuda.synchronize()
    assert bool((gx[Min:] == CANARY).all()), "gradient wrote past the end of gx"
    return gx[:Min]


def _fwd(dims, op):
    return _run_fwd(dims, _dev(op.x), _dev(op.pscale), _dev(op.pshift), _dev(op.w))


def _bwd(dims, op):
    return _run_bwd(dims, _dev(op.g), dims[4], _dev(op.wt), _dev(op.x), _dev(op.pscale), _dev(op.pshift))


@pytest.mark.parametrize("row", tr.ROWS, ids=str)
def test_transition_against_the_fp64_restatement(row):
    """Forward and input gradient of one row on its exact leg, bit for bit, and on the gaussian leg under the derived bound
    (ratio printed); a second call gives the same bits; the canary rows behind the outputs stay.  Rows, names and operands
    are those of tests/test_dense_transition_cpu.py, where the emulation passes them and every premise is asserted on the
    reference alone."""
    name = tr.row_name(*row)
    exact, _ = tr.legs_of(row)
    r = tr.reference_row(row, exact)
    y, gx = _fwd(row, r.ops), _bwd(row, r.ops)
    d1.compare_exact(name + "/" + exact + "/fwd", y, r.fwd)
    d1.compare_exact(name + "/" + exact + "/bwd", gx, r.bwd)
    r = tr.reference_row(row, "gaussian")
    y, gx = _fwd(row, r.ops), _bwd(row, r.ops)
    rf, rb = d1.gaussian_ratio(y.cpu(), r.fwd), d1.gaussian_ratio(gx.cpu(), r.bwd)
    print(name, "gaussian max |err| / bound: fwd %.3f bwd %.3f" % (rf, rb))
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)
    assert _same(y, _fwd(row, r.ops)) and _same(gx, _bwd(row, r.ops))


@pytest.mark.parametrize("row", [(3, 4, 6, 72, 136), (2, 16, 18, 256, 128), (5, 2, 2, 8, 512)], ids=str)
def test_strided_gradient_equals_dense_bitwise(row):
    """g embedded at the pitches N + 8 and 4 N in buffers of NaN (what lies behind the N live columns of a row belongs to
    other slices): the gradient equals the dense call's bit for bit and holds no NaN, on the exact and the gaussian leg."""
    B, H, W, K, N = row
    Mo = B * (H // 2) * (W // 2)
    for leg in tr.legs_of(row):
        op = tr.reference_row(row, leg).ops
        want = _bwd(row, op)
        for ld in (N + 8, 4 * N):
            buf = torch.full((Mo, ld), NAN, dtype=BF16, device=DEV)
            buf[:, :N] = op.g.to(DEV)
            got = _run_bwd(row, buf, ld, _dev(op.wt), _dev(op.x), _dev(op.pscale), _dev(op.pshift))
            assert not bool(torch.isnan(got).any()), (leg, ld)
            assert _same(got, want), (leg, ld)


@pytest.mark.parametrize("row", [(3, 4, 6, 72, 136), (5, 2, 2, 8, 512)], ids=str)
def test_a_poisoned_neighbour_image_stays_in_its_rows(row):
    """Image 1 of the batch is +inf in x (a NaN there would be clamped to +0 by the prologue, as specified) and NaN in g;
    the rows behind the last image, which the clamped reads of a tile's tail must not reach, and the rows behind g are
    NaN: the outputs of the other images are unchanged in bits and finite, while image 1's own y is not."""
    B, H, W, K, N = row
    Min, Mo = B * H * W, B * (H // 2) * (W // 2)
    op = tr.reference_row(row, "gaussian").ops
    want_y, want_gx = _fwd(row, op), _bwd(row, op)
    x = torch.full((Min + PAD, K), NAN, dtype=BF16, device=DEV)
    x[:Min] = op.x.to(DEV)
    x[H * W:2 * H * W] = float("inf")
    g = torch.full((Mo + PAD, N), NAN, dtype=BF16, device=DEV)
    g[:Mo] = op.g.to(DEV)
    g[Mo // B:2 * Mo // B] = NAN
    y = _run_fwd(row, x, _dev(op.pscale), _dev(op.pshift), _dev(op.w))
    gx = _run_bwd(row, g, N, _dev(op.wt), x, _dev(op.pscale), _dev(op.pshift))
    img = lambda t, i: t.reshape(B, -1, t.shape[1])[i]
    for i in range(B):
        if i == 1:
            continue
        assert bool(torch.isfinite(img(y, i)).all()) and bool(torch.isfinite(img(gx, i)).all()), i
        assert _same(img(y, i), img(want_y, i)) and _same(img(gx, i), img(want_gx, i)), i
    assert not bool(torch.isfinite(img(y, 1)).all())               # and the poison did arrive where it belongs


def test_transition_refuses_and_leaves_outputs_untouched():
    """K = 12, N = 20, K or N = 2056, odd H, odd W, H = 0, B = 0, every NULL pointer, misaligned bf16 pointers and tables,
    ldg below N or no multiple of 8: ADIL_EINVAL, canaries intact; then the accepted forms write exactly their extent."""
    o, lib = ops(), _lib()
    big = torch.zeros(64 * 2064, dtype=BF16, device=DEV)
    tab = torch.zeros(2064, dtype=torch.float32, device=DEV)
    out = torch.full((64 * 2064,), CANARY, dtype=BF16, device=DEV)
    P, S = o._ptr, o._stream
    odd = lambda t: t.data_ptr() + 2                          # a table address that is no multiple of 4

    def fwd(x, ps, pb, w, y, B=1, H=8, W=8, K=16, N=16):
        return lib.adil_dense_transition_fwd(x, ps, pb, w, y, B, H, W, K, N, S())

    def bwd(g, wt, xin, ps, pb, gx, ldg=16, B=1, H=8, W=8, K=16, N=16):
        return lib.adil_dense_transition_bwd(g, ldg, wt, xin, ps, pb, gx, B, H, W, K, N, S())

    good_f = [P(big), P(tab), P(tab), P(big), P(out)]
    good_b = [P(big), P(big), P(big), P(tab), P(tab), P(out)]
    for d in (dict(K=12), dict(N=20), dict(K=2056), dict(N=2056), dict(K=0), dict(K=4), dict(N=4), dict(H=7), dict(W=5),
              dict(H=0), dict(W=0), dict(B=0), dict(B=-1), dict(B=2 ** 15, H=2 ** 8, W=2 ** 8)):
        assert fwd(*good_f, **d) == EINVAL, d
        assert bwd(*good_b, **dict(d, ldg=4096)) == EINVAL, d
    for ldg in (8, 12, 17, 20, 0, -16):
        assert bwd(*good_b, ldg=ldg) == EINVAL, ldg
    for i in range(len(good_f)):
        a = list(good_f)
        a[i] = None
        assert fwd(*a) == EINVAL, i
        a[i] = odd(tab) if i in (1, 2) else (P(out[4:]) if i == 4 else P(big[4:]))
        assert fwd(*a) == EINVAL, i
    for i in range(len(good_b)):
        a = list(good_b)
        a[i] = None
        assert bwd(*a) == EINVAL, i
        a[i] = odd(tab) if i in (3, 4) else (P(out[4:]) if i == 5 else P(big[4:]))
        assert bwd(*a) == EINVAL, i
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    # the accepted forms: tables at a 4-byte (not 16-byte) address; a pitch above N
    assert fwd(P(big), P(tab[1:]), P(tab[3:]), P(big), P(out)) == 0
    torch.cuda.synchronize()
    assert bool((out[:16 * 16] == 0).all()) and bool((out[16 * 16:] == CANARY).all())
    assert bwd(P(big), P(big), P(big), P(tab[1:]), P(tab[2:]), P(out), ldg=24) == 0
    torch.cuda.synchronize()
    assert bool((out[:64 * 16] == 0).all()) and bool((out[64 * 16:] == CANARY).all())


AUTOGRAD_ROWS = [(2, 14, 14, 96, 128), (3, 6, 4, 256, 128), (1, 10, 12, 24, 40)]


def _nchw(t, b, h, w):
    return t.to(DEV).reshape(b, h, w, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("row", AUTOGRAD_ROWS, ids=str)
def test_autograd_function_equals_the_c_abi_bitwise(row):
    """ops.dense_transition on NCHW-shaped channels_last tensors: the very bits of the C-ABI calls, x saved itself (no
    copy), the output a channels_last view; the same with the incoming gradient given as the first N channels of a wider
    channels_last tensor, which is read in place (no contiguous copy: `_nhwc_grad` is not called); ValueError on a wrong
    dtype, layout, device or an odd H."""
    o = ops()
    b, h, w, k, n = row
    op = tr.operands("autograd/%s" % (row,), "gaussian", row)
    want_y, want_gx = _fwd(row, op), _bwd(row, op)
    x = _nchw(op.x, b, h, w).requires_grad_(True)
    args = (_dev(op.pscale), _dev(op.pshift), _dev(op.w), _dev(op.wt))
    y = o.dense_transition(x, *args)
    assert y.shape == (b, n, h // 2, w // 2) and y.dtype == BF16 and y.permute(0, 2, 3, 1).is_contiguous()
    assert _same(y.detach().permute(0, 2, 3, 1).reshape(-1, n), want_y)
    assert x.data_ptr() in [t.data_ptr() for t in y.grad_fn.saved_tensors]           # x itself, not a copy
    g = _nchw(op.g, b, h // 2, w // 2)
    (gx,) = torch.autograd.grad(y, (x,), g, retain_graph=True)
    assert gx.shape == x.shape and gx.permute(0, 2, 3, 1).is_contiguous()
    assert _same(gx.permute(0, 2, 3, 1).reshape(-1, k), want_gx)
    # the gradient as a channel slice of a wider buffer whose other channels are NaN
    wide = torch.full((b, h // 2, w // 2, n + 40), NAN, dtype=BF16, device=DEV)
    wide[..., :n] = op.g.to(DEV).reshape(b, h // 2, w // 2, n)
    gs = wide.permute(0, 3, 1, 2)[:, :n]
    assert not gs.permute(0, 2, 3, 1).is_contiguous()
    copies, real = [], o._nhwc_grad
    o._nhwc_grad = lambda t: (copies.append(1), real(t))[1]
    try:
        (gx2,) = torch.autograd.grad(y, (x,), gs, retain_graph=True)
        assert copies == []
        (gx3,) = torch.autograd.grad(y, (x,), g.contiguous())     # NCHW-contiguous: the one copy of `_nhwc_grad`
        assert copies == [1]
    finally:
        o._nhwc_grad = real
    assert _same(gx2.permute(0, 2, 3, 1).reshape(-1, k), want_gx)
    assert _same(gx3.permute(0, 2, 3, 1).reshape(-1, k), want_gx)
    with pytest.raises(ValueError):
        o.dense_transition(x.float(), *args)
    with pytest.raises(ValueError):
        o.dense_transition(x[:, :k - 8], *args)
    with pytest.raises(ValueError):
        o.dense_transition(x[:, :, :h - 1], *args)                  # odd H
    with pytest.raises(ValueError):
        o.dense_transition(x[:, :, :, :w - 1], *args)               # odd W
    with pytest.raises(ValueError):
        o.dense_transition(x.detach().cpu(), *args)
    with pytest.raises(ValueError):
        o.dense_transition(x, args[0].double(), *args[1:])
    with pytest.raises(ValueError):
        o.dense_transition(x, args[0].cpu(), *args[1:])
    with pytest.raises(ValueError):
        o.dense_transition(x, args[0], args[1], args[2].t(), args[3])
    with pytest.raises(ValueError):                                  # NCHW-contiguous x: it would have to be copied
        o.dense_transition(x.detach().contiguous(), *args)


def test_transition_in_a_captured_graph():
    """One transition's forward + input gradient captured in a graph — a single chain on one stream, no parallel branches
    — and replayed on two input sets equals the eager result bit for bit."""
    o = ops()
    row = (4, 14, 14, 512, 256)
    b, h, w, k, n = row
    op, op2 = tr.operands("graph", "gaussian", row), tr.operands("graph/2", "gaussian", row)
    args = (_dev(op.pscale), _dev(op.pshift), _dev(op.w), _dev(op.wt))

    def run(x, g):
        y = o.dense_transition(x, *args)
        (gx,) = torch.autograd.grad(y, x, g)
        return y, gx

    eager = [tuple(t.detach().clone() for t in run(_nchw(q.x, b, h, w).requires_grad_(True), _nchw(q.g, b, h // 2, w // 2)))
             for q in (op, op2)]
    xs = _nchw(op.x, b, h, w).clone(memory_format=torch.preserve_format).requires_grad_(True)
    gs = _nchw(op.g, b, h // 2, w // 2).clone(memory_format=torch.preserve_format)
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
            gs.copy_(_nchw(q.g, b, h // 2, w // 2))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(ys.detach().permute(0, 2, 3, 1), want_y.permute(0, 2, 3, 1))
        assert _same(gxs.permute(0, 2, 3, 1), want_gx.permute(0, 2, 3, 1))


def test_odd_sizes_keep_the_path_they_have(monkeypatch):
    """An `_OwnTransition` with the switch on and an input of odd H: the 1x1 kernel and the library pool, bit for bit what
    the module gives with the switch off, and `ops.dense_transition` is not called; an even input goes through it once."""
    from dl_attack_on_imagenet_amd import zoo
    o = ops()
    torch.manual_seed(0)
    net = zoo.DenseNet(num_classes=4).eval()
    zoo.use_own_dense_pointwise_(net)
    t1 = net.features.transition1.to(device=DEV, dtype=BF16)
    gen = torch.Generator().manual_seed(1)
    cl = lambda t: t.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    odd, even = cl(torch.randn(2, 256, 7, 8, generator=gen)), cl(torch.randn(2, 256, 6, 8, generator=gen))
    calls, real = [], o.dense_transition
    monkeypatch.setattr(o, "dense_transition", lambda *a: (calls.append(1), real(*a))[1])
    with torch.no_grad():
        off_odd, off_even = t1(odd), t1(even)
        assert zoo.use_own_dense_transition_(net) == 3
        assert not t1._pools_first(odd) and t1._pools_first(even)
        assert _same(t1(odd), off_odd) and calls == []
        on_even = t1(even)
    assert calls == [1] and on_even.shape == off_even.shape == (2, 128, 3, 4)
    assert on_even.is_contiguous(memory_format=torch.channels_last) and bool(torch.isfinite(on_even).all())


# ---------------------------------------------------------------------------------------------------------------- network
def randomised_checkpoint(path, seed=5, num_classes=1000):
    """The recipe of tests/test_gpu_dense_block.randomised_checkpoint, restated: a seeded DenseNet-121 state_dict with
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
    logits = model(x).float()
    (g,) = torch.autograd.grad(logits.square().sum(), x)
    return logits.detach(), g.detach().float()


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32-input", "bf16-input"])
def test_stem_wiring_equals_the_fused_stem_bitwise(tmp_path, dtype):
    """The `own_dense_stem` network hands its first dense block the very bits `zoo._FusedStem(conv0, norm0, mean, std)`
    produces on the same weights, and the input gradient of a weighted sum of that tensor is the same in bits, for fp32 and
    bf16 image tensors: the switch is wiring, the stem kernels are the ResNets'."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import zoo
    images, _ = structured_images(3, classes=3, seed=3, size=64)
    path = randomised_checkpoint(os.path.join(str(tmp_path), "densenet_random_bn.pt"), num_classes=8)
    kw = dict(num_classes=8, seed=5, weights=path, device=DEV)
    fp32 = zoo.build_classifier("densenet121", **kw)
    feat = fp32[1].features
    ref = zoo._FusedStem(feat.conv0, feat.norm0, MEAN, STD).to(DEV)
    own = zoo.build_classifier("densenet121", dtype=BF16, channels_last=True, own_dense_stem=True, **kw)
    assert len(own) == 1 and isinstance(own[0].features, zoo._OwnDenseStem)
    seen = []
    handle = own[0].features.denseblock1.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    x = images.to(DEV).to(dtype).requires_grad_(True)
    own(x)
    handle.remove()
    (got,) = seen
    want = ref(x)
    assert got.shape == want.shape == (3, 64, 16, 16) and got.dtype == BF16
    assert _same(got.detach().permute(0, 2, 3, 1), want.detach().permute(0, 2, 3, 1))
    g = torch.randn(want.shape, generator=torch.Generator().manual_seed(2)).to(DEV).bfloat16()
    g = g.contiguous(memory_format=torch.channels_last)
    (g_own,) = torch.autograd.grad(got, x, g, retain_graph=True)
    (g_ref,) = torch.autograd.grad(want, x, g)
    assert g_own.dtype == g_ref.dtype == dtype and g_own.shape == x.shape and float(g_ref.abs().max()) > 0
    assert torch.equal(g_own, g_ref)


def test_densenet_on_all_five_dense_switches(tmp_path, monkeypatch):
    """All five dense switches on 4 structured images at 64 x 64 and a checkpoint with randomised BatchNorm statistics (the
    fixture recipe of test_densenet_on_the_dense_block_path, restated): the logits against the fp32 network within the
    bf16 depth bound of 121 layers, the input gradient no further from the fp32 network's than 1.5 x the distance of the
    plain bf16 network; each of the 3 transitions under the elementwise gaussian bound on its ACTUAL input; per forward
    F.conv2d, F.avg_pool2d, F.max_pool2d and torch.cat are called 0 times and F.batch_norm once (norm5); two fresh builds
    give bitwise equal logits and input gradients; each new switch alone on top of the three earlier ones meets the first
    two criteria too.
    Recorded on an MI355X: the transitions at 0.948 / 0.895 / 0.785 of their elementwise bound (256 -> 128 at 16 x 16, 512 ->
    256 at 8 x 8, 1024 -> 512 at 4 x 4); mean |logit error| 0.00528 plain bf16 / 0.00263 five switches, rms logit 0.6155,
    bound 0.02645; input-gradient relative error 0.1400 plain bf16 / 0.1201 five switches; three switches + transition
    0.00277 / 0.1321, three switches + stem 0.00258 / 0.1192 (the plain bf16 network runs library convolutions, which are
    not reproducible call to call: its figures move in the last digit)."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import zoo
    size = 64
    images, _ = structured_images(4, classes=4, seed=3, size=size)
    path = randomised_checkpoint(os.path.join(str(tmp_path), "densenet_random_bn.pt"))
    kw = dict(num_classes=1000, seed=5, weights=path, device=DEV)
    x = images.to(DEV)
    lr, gr = _forward_and_gradient(zoo.build_classifier("densenet121", **kw), x)
    kw.update(dtype=BF16, channels_last=True)
    l0, g0 = _forward_and_gradient(zoo.build_classifier("densenet121", **kw), x.bfloat16())
    rms = float(lr.square().mean().sqrt())
    bound = _bf16_depth_bound(121) * rms
    rel = lambda g: float((g - gr).norm() / gr.norm())
    e0, r0 = float((l0 - lr).abs().mean()), rel(g0)
    assert float(gr.abs().max()) > 0
    three = dict(own_dense_pointwise=True, own_dense_conv=True, own_dense_block=True)
    five = dict(three, own_dense_transition=True, own_dense_stem=True)
    own = zoo.build_classifier("densenet121", **five, **kw)
    assert sum(isinstance(m, zoo._OwnDenseBlock) for m in own.modules()) == 4
    transitions = [m for m in own.modules() if isinstance(m, zoo._OwnTransition)]
    assert len(transitions) == 3 and all(m.pool_first for m in transitions)
    seen = []
    flat = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1])

    def restate(mod, args, out):
        xin = args[0]
        assert xin.dtype == BF16 and xin.is_contiguous(memory_format=torch.channels_last)
        dims = (xin.shape[0], xin.shape[2], xin.shape[3], mod.cin, mod.cout)
        o = tr.tr_fwd(Arith(), dims, flat(xin).cpu(), mod.pscale.cpu(), mod.pshift.cpu(),
                      mod.conv.weight.detach().reshape(mod.cout, mod.cin).cpu())
        seen.append(dims + (d1.gaussian_ratio(flat(out).cpu(), o),))

    handles = [m.register_forward_hook(restate) for m in transitions]
    l1, g1 = _forward_and_gradient(own, x.bfloat16())
    for h in handles:
        h.remove()
    assert [s[:5] for s in seen] == [(4, h * size // 224, h * size // 224, k, n) for h, k, n in tr.NETWORK_TRANSITIONS]
    for *dims, ratio in seen:
        print("transition %s: max |err| / bound %.3f" % (tuple(dims), ratio))
        assert ratio <= 1.0, (dims, ratio)
    e1, r1 = float((l1 - lr).abs().mean()), rel(g1)
    print("logit error vs fp32: plain bf16 %.5f five switches %.5f, rms %.4f, bound %.5f; input gradient relative error vs "
          "fp32: plain bf16 %.4f five switches %.4f" % (e0, e1, rms, bound, r0, r1))
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all() and g1.shape == x.shape and float(g1.abs().max()) > 0
    assert e1 <= bound, (e0, e1, rms)
    assert r1 <= 1.5 * r0, (r0, r1)
    counts = OrderedDict()
    with monkeypatch.context() as mp:
        for owner, name in ((F, "conv2d"), (F, "avg_pool2d"), (F, "max_pool2d"), (torch, "cat"), (F, "batch_norm")):
            counts[name] = []
            mp.setattr(owner, name, lambda *a, _real=getattr(owner, name), _c=counts[name], **k: (_c.append(1), _real(*a, **k))[1])
        with torch.no_grad():
            own(x.bfloat16())
        got = {k: len(v) for k, v in counts.items()}
        assert got == dict(conv2d=0, avg_pool2d=0, max_pool2d=0, cat=0, batch_norm=1), got
        _forward_and_gradient(own, x.bfloat16())
        got = {k: len(v) for k, v in counts.items()}
        assert got == dict(conv2d=0, avg_pool2d=0, max_pool2d=0, cat=0, batch_norm=2), got
    again = zoo.build_classifier("densenet121", **five, **kw)
    l2, g2 = _forward_and_gradient(again, x.bfloat16())
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    for name in ("own_dense_transition", "own_dense_stem"):
        one = zoo.build_classifier("densenet121", **dict(three, **{name: True}), **kw)
        l3, g3 = _forward_and_gradient(one, x.bfloat16())
        e3, r3 = float((l3 - lr).abs().mean()), rel(g3)
        print("three switches + %s: logit error %.5f, input gradient relative error %.4f" % (name, e3, r3))
        assert torch.isfinite(l3).all() and torch.isfinite(g3).all()
        assert e3 <= bound, (name, e0, e3, rms)
        assert r3 <= 1.5 * r0, (name, r0, r3)
