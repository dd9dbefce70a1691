"""What stands between the DenseNet-121 kernels and the attack: ops.DenseBlockFunction (channel offsets, the per-layer mids,
the reverse walk with accumulate = 1, the reuse of one mid under no_grad), ops.DenseTransitionFunction with `_strided_rows`
(its gradient read in place from the next block's gradient buffer at pitch Ctot), zoo._OwnDenseStem.forward(skip_last=True),
zoo.DenseNet.forward with head32, the tables of zoo._OwnDenseHead, and ops.StemFunction.backward on the non-contiguous slice
gbuf[..., :64].  The product (zoo.build_classifier("densenet121") with all six own_dense_* switches; library convolution,
BatchNorm, linear, the three poolings and torch.cat patched to raise) against the straight-line tape of
tests/densenet_tape.py run on the C ABI with contiguous operands of its own:

(a) the eight feature points (the pooled stem output, four block outputs, three transition outputs), the fp32 logits, the
    gradient entering each of the eight points and the gradient with respect to the image, bit for bit, on both image
    shapes, with an fp32 and with a bf16 image; a first mismatch names the point;
(b) every step of such a tape run against its fp64 restatement on the step's actual inputs, within the derived
    element-wise bounds of the reference modules (ratio <= 1; the stem's pooling pair and the head's gx bit for bit);
(c) the other routes into the same kernels: engine.input_gradient alone and inside classifier_batch_bucket(4);
    own_dense_head="inference" inside engine.precise_head; the five-switch network without own_dense_block (torch.cat
    path, forward only: autograd's summation order is not specified); a forward under torch.no_grad(); two fresh builds;
(d) three mutants of the product's block backward that keep every pointer, width and pitch legal: (a) must name each of
    them at the first gradient point it reaches; what the loose recipe of
    tests/test_gpu_dense_head.py::test_densenet_on_all_six_dense_switches makes of them is printed, not asserted.

The tape itself is held to the fp64 torch modules by tests/test_densenet_wiring_cpu.py, which also asserts that every ReLU of
the reference tape is alive.  profiles/densenet_wiring.md has the measured values.  Measured on the MI355X: (a) and (c) equal
in every bit; (b) worst max err / bound 0.964 stem_fwd, 0.934 stem_bwd, 0.990 d1_fwd, 0.988 d1_bwd, 0.842 d3_fwd, 0.966
d3_bwd, 0.952 tr_fwd, 0.974 tr_bwd, 0.319 head_fwd, 0.108 head_bwd, the pooling pair equal; (d) the three mutants reported at
the gradients entering the outputs of transition 3, 2 and 1, while the loose recipe (margin 0.3723) scores the sound
product 0.1964 and the mutants 0.1966, 0.2203 and 0.6271: the first two inside its margin.  Each test takes 0.15 - 1.8 s; the
loose-recipe record 5.9 s (the plain bf16 network's first pass: the library's convolution search)."""
import os
import time

import pytest
import torch
import torch.nn.functional as F

import classifier_reference as R
import densenet_tape as T
from classifier_reference import BF16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMAGE_GRADIENT = "gradient with respect to the image"
N_LAYERS = sum(T.REAL)
COUNTS = {"adil_stem_conv_fwd": 1, "adil_maxpool_fwd": 1, "adil_stem_pool_bwd": 1, "adil_stem_conv_bwd": 1,
          "adil_dense1x1_fwd_ld": N_LAYERS, "adil_dense3x3_fwd_ld": N_LAYERS, "adil_dense3x3_bwd_ld": N_LAYERS,
          "adil_dense1x1_bwd_ld": N_LAYERS, "adil_dense_transition_fwd": 3, "adil_dense_transition_bwd": 3,
          "adil_bn_pool_head_fwd": 1, "adil_bn_pool_head_bwd": 1}
SIX = dict(own_dense_pointwise=True, own_dense_conv=True, own_dense_block=True, own_dense_transition=True, own_dense_stem=True,
           own_dense_head=True)
SHAPE_IDS = ["2x96x32", "1x94x62"]


def lib():
    from dl_attack_on_imagenet_amd import _lib
    return _lib.load()


def zoo():
    from dl_attack_on_imagenet_amd import zoo as z
    return z


# ------------------------------------------------------------------------------------------------- network and tapes
_SHARED = {}


def shared(key, make):
    """Computed once and left unchanged."""
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


def plain_net():
    return shared("net", lambda: T.make_net(T.REAL)[0])


def tables(device):
    return shared(("tables", device), lambda: T.layer_tables(plain_net(), product=True, device=device))


def inputs(shape, dtype):
    x, g = T.make_inputs(shape)
    return x.to(dtype).contiguous(), g


def reference_tape(shape, dtype):
    """The tape over the fp64 restatements with the kernels' roundings, on the CPU: the premises are asserted on it."""
    def make():
        x, g = inputs(shape, dtype)
        tape = T.run_tape(T.Restate(R.Arith()), tables("cpu"), x, g)
        T.assert_premises(tape, tables("cpu"), "reference tape %s" % (shape,))
        return tape
    return shared(("reference", shape, dtype), make)


def abi_tape(shape, dtype, g_logits=None, keep_log=False):
    be = T.Abi(lib(), keep_log=keep_log)
    x, g = inputs(shape, dtype)
    tape = T.run_tape(be, tables(DEV), x.to(DEV), (g if g_logits is None else g_logits).to(DEV))
    torch.cuda.synchronize()
    return tape, be


def shared_tape(shape, dtype):
    def make():
        reference_tape(shape, dtype)                                   # premises first, on the reference alone
        return abi_tape(shape, dtype)[0]
    return shared(("abi", shape, dtype), make)


def checkpoint(tmp_path):
    path = os.path.join(str(tmp_path), "densenet_wiring.pt")
    torch.save(plain_net().state_dict(), path)
    return path


def build_product(path, **switches):
    kw = dict(SIX)
    kw.update(switches)
    return zoo().build_classifier("densenet121", num_classes=T.CLASSES, weights=path, device=DEV, dtype=BF16, channels_last=True, **kw)


def refuse_the_library(mp, cat=True):
    def refuse(name):
        def fn(*a, **k):
            raise AssertionError("library call: %s" % name)
        return fn
    for name in ("conv2d", "batch_norm", "linear", "max_pool2d", "avg_pool2d", "adaptive_avg_pool2d"):
        mp.setattr(F, name, refuse("F." + name))
    if cat:
        mp.setattr(torch, "cat", refuse("torch.cat"))


class Spy:
    """The loaded library with every call counted by entry point."""

    def __init__(self, loaded):
        self._loaded, self.calls = loaded, {}

    def __getattr__(self, name):
        fn = getattr(self._loaded, name)
        if not name.startswith("adil_"):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


class Run:
    pass


def names(grads=True):
    pts = T.point_names()
    return pts + ["logits"] + ((["gradient at the " + n for n in reversed(pts)] + [IMAGE_GRADIENT]) if grads else [])


def product_run(model, x, g_logits, mp, cat=True, no_grad=False):
    """Forward (and input gradient, with g_logits) of the product with the library patched to raise and the C ABI observed:
    the eight points (a forward pre-hook on denseblock1 for the stem's pooled output, forward hooks on the four blocks and
    three transitions; NHWC), the gradients entering them (tensor hooks), the logits, the gradient with respect to x, the
    calls per entry point."""
    from dl_attack_on_imagenet_amd import _lib
    r, hooks = Run(), []
    r.points, r.grads = [None] * 8, [None] * 8
    children = dict(model[0].features.named_children())
    order = [n for n in children if n.startswith(("denseblock", "transition"))]
    assert len(order) == 7 and order[0] == "denseblock1"

    def keep(i, t):
        r.points[i] = t.detach().permute(0, 2, 3, 1)
        if t.requires_grad:
            t.register_hook(lambda g, i=i: r.grads.__setitem__(i, g.detach().permute(0, 2, 3, 1).clone()))

    hooks.append(children["denseblock1"].register_forward_pre_hook(lambda m, a: keep(0, a[0])))
    for i, n in enumerate(order):
        hooks.append(children[n].register_forward_hook(lambda m, a, out, i=i: keep(i + 1, out)))
    spy = Spy(lib())
    xi = x.detach().clone()
    with mp.context() as m:
        refuse_the_library(m, cat=cat)
        m.setattr(_lib, "_lib", spy)
        if no_grad:
            with torch.no_grad():
                logits = model(xi)
            gx = None
        elif g_logits is None:
            logits, gx = model(xi), None
        else:
            xi.requires_grad_(True)
            logits = model(xi)
            (gx,) = torch.autograd.grad(logits, xi, g_logits)
    for hk in hooks:
        hk.remove()
    torch.cuda.synchronize()
    r.logits, r.grad, r.calls, r.x = logits.detach(), gx, spy.calls, xi
    return r


def _same(a, b):
    return a is not None and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def first_mismatch(r, tape, grads=True):
    """None, or the name of the first tensor of the product that differs from the tape's (values: +0 equals -0), in the
    order of `names`: the points in forward order, the logits, then the gradients from the head back to the image."""
    got = r.points + [r.logits] + ((list(reversed(r.grads)) + [r.grad]) if grads else [])
    want = tape.points + [tape.logits] + ((list(reversed(tape.grads)) + [tape.grad]) if grads else [])
    for n, a, b in zip(names(grads), got, want):
        assert float(b.float().abs().sum()) > 0, f"the tape's {n} is zero: the comparison would be vacuous"
        if not _same(a, b):
            return n
    return None


def assert_run_premises(model, r, x):
    """The run exercised what it was meant to: the rewritten modules and every kernel path, nothing else."""
    z = zoo()
    net = model[0]
    count = lambda kind: sum(isinstance(m, kind) for m in net.modules())
    assert len(model) == 1 and isinstance(net, z.DenseNet) and net.head32_on and isinstance(net.head32, z._OwnDenseHead)
    assert isinstance(net.features, z._OwnDenseStem)
    assert (count(z._OwnDenseBlock), count(z._OwnDenseLayer), count(z._OwnGrowthConv), count(z._OwnTransition)) == (4, N_LAYERS, N_LAYERS, 3)
    assert all(m.pool_first for m in net.modules() if isinstance(m, z._OwnTransition))
    assert r.calls == COUNTS, r.calls
    for n, t in zip(T.point_names(), r.points):
        assert t is not None and t.dtype == BF16, n
    for n, t in zip(T.point_names(), r.grads):
        assert t is not None and t.dtype == BF16 and bool(torch.isfinite(t.float()).all()), "gradient at the " + n
    assert r.logits.dtype == F32 and r.logits.shape == (x.shape[0], T.CLASSES)
    assert r.grad.dtype == x.dtype and r.grad.shape == x.shape and r.grad.is_contiguous()
    assert bool(torch.isfinite(r.grad.float()).all()) and all(float(r.grad[:, c].float().abs().max()) > 0 for c in range(3))


# ------------------------------------------------------------------------------------- (a) the product and the tape
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32_image", "bf16_image"])
@pytest.mark.parametrize("shape", T.SHAPES, ids=SHAPE_IDS)
def test_densenet_equals_the_tape_bitwise(shape, dtype, tmp_path, monkeypatch):
    t0 = time.time()
    tape = shared_tape(shape, dtype)
    shares = T.assert_premises(tape, tables(DEV), "C-ABI tape %s" % (shape,))
    if dtype == F32:
        lo, hi = min(shares, key=lambda s: s[1]), max(shares, key=lambda s: s[1])
        print(f"{shape}: {len(shares)} ReLU shares of the C-ABI tape, lowest {lo[1]:.4f} at the {lo[0]}, highest {hi[1]:.4f} at the {hi[0]}")
    model = build_product(checkpoint(tmp_path))
    x, g = inputs(shape, dtype)
    r = product_run(model, x.to(DEV), g.to(DEV), monkeypatch)
    assert_run_premises(model, r, x)
    bad = first_mismatch(r, tape)
    assert bad is None, f"{shape} {dtype}: the product and the C-ABI tape differ first at the {bad}"
    print(f"{shape} {dtype}: 8 feature points, the logits, 8 gradient points and the image gradient equal the tape's; "
          f"{time.time() - t0:.2f} s")


# --------------------------------------------------------------------------- (b) the tape's steps are the restatements
@pytest.mark.parametrize("shape,dtype", [(T.SHAPES[0], F32), (T.SHAPES[1], BF16)], ids=["2x96x32_fp32", "1x94x62_bf16"])
def test_every_tape_step_is_within_the_bound_of_its_restatement(shape, dtype):
    t0 = time.time()
    reference_tape(shape, dtype)
    tape, be = abi_tape(shape, dtype, keep_log=True)
    worst, count = T.step_ratios(be.log)
    for name in T.STEPS:
        print(f"{shape}: {name:9s} {count.get(name, 0):3d} steps, worst max err / bound = {worst.get(name, float('nan')):.3f}")
    assert count == T.step_counts(T.REAL)
    for name, q in worst.items():
        assert q <= 1.0, f"{shape}: a {name} step is {q:.3f} times its bound away from the restatement"
    print(f"{shape}: {time.time() - t0:.2f} s")


# ------------------------------------------------------------------------------------------- (c) the other routes
def test_the_learners_route_equals_the_tape_bitwise(tmp_path, monkeypatch):
    """engine.input_gradient(model, x, labels, "ce", ...) against the tape driven with the loss gradient torch computes
    from the tape's OWN logits; then inside classifier_batch_bucket(4): 2 rows padded to 4 with zero images (the padding
    itself is a torch.cat, which stays allowed there)."""
    from dl_attack_on_imagenet_amd import engine
    t0 = time.time()
    shape = T.SHAPES[0]
    model = build_product(checkpoint(tmp_path))
    x, _ = inputs(shape, F32)
    x = x.to(DEV)
    labels = torch.tensor([3, 0], device=DEV)
    loss = ("ce", -1.0, 0.0, "mean")
    fwd = shared_tape(shape, F32)
    tl = fwd.logits.detach().clone().requires_grad_(True)
    (g_logits,) = torch.autograd.grad(engine.attack_loss(tl, labels, *loss), tl)
    assert g_logits.dtype == F32 and bool((g_logits != 0).all())
    tape, _ = abi_tape(shape, F32, g_logits=g_logits)
    assert torch.equal(tape.logits, fwd.logits)
    with monkeypatch.context() as mp:
        refuse_the_library(mp)
        out, ls, gx = engine.input_gradient(model, x, labels, *loss)
    with monkeypatch.context() as mp:
        refuse_the_library(mp, cat=False)
        with engine.classifier_batch_bucket(4):
            out4, ls4, gx4 = engine.input_gradient(model, x, labels, *loss)
    torch.cuda.synchronize()
    for o, g in ((out, gx), (out4, gx4)):
        assert o.dtype == F32 and o.shape == (2, T.CLASSES) and g.dtype == F32 and g.shape == x.shape and g.is_contiguous()
    assert torch.equal(out, tape.logits), "the learner's logits differ from the tape's"
    assert torch.equal(gx, tape.grad), "the learner's image gradient differs from the tape's"
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().sum()) > 0
    assert torch.equal(out4, out) and torch.equal(ls4, ls), "padding the batch to 4 rows changes the logits of the real rows"
    assert torch.equal(gx4, gx), "padding the batch to 4 rows changes the image gradient of the real rows"
    print(f"learner's route: logits and image gradient equal the tape's, with and without the batch bucket; {time.time() - t0:.2f} s")


def test_the_inference_head_gives_the_tapes_logits(tmp_path, monkeypatch):
    """own_dense_head="inference": inside engine.precise_head the network runs the trunk up to norm5 and the head kernels,
    and its logits are the tape's."""
    from dl_attack_on_imagenet_amd import engine
    t0 = time.time()
    model = build_product(checkpoint(tmp_path), own_dense_head="inference")
    assert not model[0].head32_on
    for shape in T.SHAPES:
        tape = shared_tape(shape, BF16)
        x, _ = inputs(shape, BF16)
        with engine.precise_head(model):
            assert model[0].head32_on
            r = product_run(model, x.to(DEV), None, monkeypatch, no_grad=True)
        assert not model[0].head32_on
        assert r.calls == {k: v for k, v in COUNTS.items() if "bwd" not in k}, r.calls
        bad = first_mismatch(r, tape, grads=False)
        assert bad is None, f"{shape}: the inference head's network and the tape differ first at the {bad}"
    print(f"inference head: 8 feature points and the logits equal the tape's on both shapes; {time.time() - t0:.2f} s")


def test_the_torch_cat_path_equals_the_tapes_forward_bitwise(tmp_path, monkeypatch):
    """The five-switch network with own_dense_block=False: every layer on torch.cat's copies through the plain entry points.
    Forward only: its gradient sums are autograd's, whose order is not specified."""
    t0 = time.time()
    z = zoo()
    model = build_product(checkpoint(tmp_path), own_dense_block=False)
    assert sum(isinstance(m, z._OwnDenseBlock) for m in model.modules()) == 0
    assert sum(isinstance(m, z._DenseBlock) for m in model.modules()) == 4
    for shape in T.SHAPES:
        tape = shared_tape(shape, F32)
        x, g = inputs(shape, F32)
        r = product_run(model, x.to(DEV), g.to(DEV), monkeypatch, cat=False)
        assert r.calls.get("adil_dense1x1_fwd") == N_LAYERS and r.calls.get("adil_dense3x3_fwd") == N_LAYERS, r.calls
        assert "adil_dense1x1_fwd_ld" not in r.calls and r.calls.get("adil_dense_transition_fwd") == 3
        bad = first_mismatch(r, tape, grads=False)
        assert bad is None, f"{shape}: the torch.cat path and the tape differ first at the {bad}"
        assert bool(torch.isfinite(r.grad).all()) and float(r.grad.abs().sum()) > 0
        rel = float((r.grad.double() - tape.grad.double()).norm() / tape.grad.double().norm())
        print(f"{shape}: torch.cat path, image gradient (autograd's sums) relative to the tape's: {rel:.4f} (printed, not asserted)")
    print(f"torch.cat path: 8 feature points and the logits equal the tape's on both shapes; {time.time() - t0:.2f} s")


def test_a_forward_without_grad_has_the_bits_of_the_forward_with_grad(tmp_path, monkeypatch):
    """Under torch.no_grad() ops.DenseBlockFunction keeps nothing and reuses ONE mid for all layers of a block."""
    t0 = time.time()
    model = build_product(checkpoint(tmp_path))
    for shape, dtype in ((T.SHAPES[0], BF16), (T.SHAPES[1], F32)):
        tape = shared_tape(shape, dtype)
        x, _ = inputs(shape, dtype)
        r = product_run(model, x.to(DEV), None, monkeypatch, no_grad=True)
        assert r.calls == {k: v for k, v in COUNTS.items() if "bwd" not in k}, r.calls
        assert not r.logits.requires_grad and all(g is None for g in r.grads)
        bad = first_mismatch(r, tape, grads=False)
        assert bad is None, f"{shape} {dtype}: the forward under no_grad and the tape differ first at the {bad}"
    print(f"no_grad forward: 8 feature points and the logits equal the tape's; {time.time() - t0:.2f} s")


def test_two_fresh_builds_agree_bitwise(tmp_path, monkeypatch):
    t0 = time.time()
    shape = T.SHAPES[0]
    path = checkpoint(tmp_path)
    x, g = inputs(shape, F32)
    a = product_run(build_product(path), x.to(DEV), g.to(DEV), monkeypatch)
    b = product_run(build_product(path), x.to(DEV), g.to(DEV), monkeypatch)
    bits32 = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits32(a.logits), bits32(b.logits)) and torch.equal(bits32(a.grad), bits32(b.grad))
    for t, u in zip(a.points + a.grads, b.points + b.grads):
        assert torch.equal(R.bits(t), R.bits(u))
    print(f"two fresh builds: logits, image gradient, 8 feature points and 8 gradient points hold the same bits; {time.time() - t0:.2f} s")


# ------------------------------------------------------------------------------------------ (d) the comparison notices
def _mutated_block_backward(which):
    """ops.DenseBlockFunction.backward with ONE mistake; pointers, widths and pitches as in the sound one.
    round_then_add: every block computes each contribution with accumulate = 0 into a contiguous temporary [M][off_i]
      (ldgx = off_i) and adds it to the gradient buffer in bf16: the order the specification excludes.
    last_layer_dropped: the block of 24 layers (denseblock3) leaves out its last layer.
    first_to_last: the block of 12 layers (denseblock2) walks its layers first to last."""
    from dl_attack_on_imagenet_amd import _lib, ops

    def backward(ctx, g):
        L = ops.DENSE_BLOCK_LAYER_OPERANDS
        n, c0, mid, growth = ctx.meta
        saved = ctx.saved_tensors
        buf, mids, flat = saved[0], saved[1:1 + n], saved[1 + n:]
        assert ctx.needs_input_grad[0]
        loaded, ptr, stream = _lib.load(), ops._ptr, ops._stream()
        b, h, w, ctot = buf.shape
        m = b * h * w
        gbuf = torch.empty((b, h, w, ctot), dtype=BF16, device=buf.device)
        gbuf.copy_(g.permute(0, 2, 3, 1))
        grows = gbuf.view(m, ctot)
        gmid = torch.empty((m, mid), dtype=BF16, device=buf.device)
        order = range(n - 1, -1, -1)
        if which == "last_layer_dropped" and n == 24:
            order = range(n - 2, -1, -1)
        if which == "first_to_last" and n == 12:
            order = range(n)
        for i in order:
            pscale, pshift, _, wt2d, scale, _, _, wp_bwd = flat[L * i:L * i + L]
            off = c0 + i * growth
            _lib.check(loaded.adil_dense3x3_bwd_ld(ptr(grows[:, off:]), ctot, ptr(wp_bwd), ptr(gmid), mid, b, h, w, mid, growth, stream),
                       "adil_dense3x3_bwd_ld")
            if which == "round_then_add":
                tmp = torch.empty((m, off), dtype=BF16, device=buf.device)
                _lib.check(loaded.adil_dense1x1_bwd_ld(ptr(gmid), mid, ptr(mids[i]), mid, ptr(scale), ptr(wt2d), ptr(buf), ctot,
                                                       ptr(pscale), ptr(pshift), ptr(tmp), off, 0, m, off, mid, 1, stream),
                           "adil_dense1x1_bwd_ld")
                grows[:, :off] += tmp
            else:
                _lib.check(loaded.adil_dense1x1_bwd_ld(ptr(gmid), mid, ptr(mids[i]), mid, ptr(scale), ptr(wt2d), ptr(buf), ctot,
                                                       ptr(pscale), ptr(pshift), ptr(gbuf), ctot, 1, m, off, mid, 1, stream),
                           "adil_dense1x1_bwd_ld")
        return (gbuf[..., :c0].permute(0, 3, 1, 2), None) + (None,) * len(flat)
    return staticmethod(backward)


# the first gradient point each mutant reaches: the input of the last block; of denseblock3; of denseblock2
MUTANTS = [("round_then_add", "gradient at the output of transition3"),
           ("last_layer_dropped", "gradient at the output of transition2"),
           ("first_to_last", "gradient at the output of transition1")]


def _mutate(mp, which):
    from dl_attack_on_imagenet_amd import ops
    mp.setattr(ops.DenseBlockFunction, "backward", _mutated_block_backward(which))


@pytest.mark.parametrize("which,expect", MUTANTS)
def test_a_mutant_of_the_product_is_reported(which, expect, tmp_path, monkeypatch):
    t0 = time.time()
    shape = T.SHAPES[0]
    tape = shared_tape(shape, F32)
    model = build_product(checkpoint(tmp_path))
    x, g = inputs(shape, F32)
    with monkeypatch.context() as mp:
        _mutate(mp, which)
        r = product_run(model, x.to(DEV), g.to(DEV), mp)
    bad = first_mismatch(r, tape)
    print(f"mutant {which}: first mismatch at the {bad}; {time.time() - t0:.2f} s")
    assert bad == expect, (bad, expect)
    r = product_run(model, x.to(DEV), g.to(DEV), monkeypatch)           # ... and the sound product is back
    assert r.calls == COUNTS and first_mismatch(r, tape) is None


def test_what_the_loose_recipe_makes_of_the_mutants(tmp_path, monkeypatch):
    """For the record (printed, not asserted): the recipe of test_densenet_on_all_six_dense_switches (the input gradient of
    sum logits^2 no further from the fp32 network's than 1.5 x the plain bf16 network's, relative) on this network and the
    2 x 3 x 96 x 32 batch, for the sound product and for the three mutants.  Measured on the MI355X: see
    profiles/densenet_wiring.md."""
    t0 = time.time()
    path = checkpoint(tmp_path)
    kw = dict(num_classes=T.CLASSES, weights=path)
    ref = zoo().build_classifier("densenet121", **kw)                   # the fp32 network, on the CPU (no convolution search)
    off = zoo().build_classifier("densenet121", dtype=BF16, channels_last=True, device=DEV, **kw)
    own = build_product(path)
    x = inputs(T.SHAPES[0], F32)[0]

    def gradient(m, xi):
        xi = xi.clone().requires_grad_(True)
        return torch.autograd.grad(m(xi).float().square().sum(), xi)[0].float().cpu()

    gr = gradient(ref, x)
    x = x.to(DEV)
    rel = lambda g: float((g - gr).norm() / gr.norm())
    r0 = rel(gradient(off, x.bfloat16()))
    print(f"loose recipe: plain bf16 network {r0:.4f}, so the margin is {1.5 * r0:.4f}; {time.time() - t0:.2f} s so far")
    for which in [None] + [m for m, _ in MUTANTS]:
        with monkeypatch.context() as mp:
            if which:
                _mutate(mp, which)
            g1 = gradient(own, x.bfloat16())
        assert bool(torch.isfinite(g1).all())
        print(f"loose recipe, {which or 'sound product'}: relative error {rel(g1):.4f} ({'inside' if rel(g1) <= 1.5 * r0 else 'outside'} "
              f"the margin)")
    print(f"loose recipe: {time.time() - t0:.2f} s")
