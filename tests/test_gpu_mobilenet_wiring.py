"""What stands between the MobileNetV2 kernels and the attack: the block logic of zoo._OwnFirstConv / _OwnDepthwise /
_OwnPointwise / _OwnInvertedResidual / _OwnHead, their tables under a cast, and the backward that autograd assembles over
17 blocks and 10 residual joins.  The product (zoo.build_classifier with all four switches, library convolution, BatchNorm,
linear, pooling and ReLU6 patched to raise) against the straight-line tape of tests/mobilenet_tape.py run on the C ABI:

(a) the 19 outputs of features[0 .. 18], the fp32 logits and the gradient with respect to the image, bit for bit, on both
    image shapes, with an fp32 and with a bf16 image;
(b) every step of such a tape run against its fp64 restatement on the step's actual inputs, within the derived
    element-wise bounds of the four reference modules (ratio <= 1);
(c) the learner's route: engine.input_gradient with the cross-entropy loss, alone and inside classifier_batch_bucket(4);
(d) the fp32 tables and the transposed weights after casts of the module;
(e) three mutants of the product that only omit or misroute an optional operand: (a) must name each of them;
(f) two fresh builds, bit for bit.

The tape itself is held to the fp64 torch modules by tests/test_mobilenet_wiring_cpu.py.  profiles/mobilenet_wiring.md has
the measured values.  Measured on the MI355X: (a), (c), (d), (f) equal in every bit; (b) worst max err / bound 0.986
first_fwd, 0.970 first_bwd, 0.995 dw_fwd and dw_bwd, 0.993 pw8_fwd, 0.995 pw8_bwd, 0.095 head_fwd, 0.119 head_bwd; (e) the
three mutants reported at the image gradient, the image gradient and features[5], while the loose recipe of
test_mobilenet_on_own_pointwise_kernels (relative gradient error against the fp32 network at most 1.5 x the plain bf16
network's 1.28 on this network) scores the sound product 1.17 and the mutants 1.10, 1.38 and 1.26: all inside its margin.
Each test takes 0.04 - 1.5 s; the loose-recipe record 7.6 s alone in a fresh process (the library's convolution search)."""
import os
import time

import pytest
import torch
import torch.nn.functional as F

import classifier_reference as R
import mobilenet_tape as T
from classifier_reference import BF16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMAGE_GRADIENT = "gradient with respect to the image"
COUNTS = {"adil_first3x3_fwd": 1, "adil_first3x3_bwd": 1, "adil_dw3x3_fwd": 17, "adil_dw3x3_bwd": 17, "adil_pw8_fwd": 34,
          "adil_pw8_bwd": 34, "adil_pool_head_fwd": 1, "adil_pool_head_bwd": 1}


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
    return shared("net", T.make_net)


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
        T.assert_premises(tape, "reference tape %s" % (shape,))
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
    path = os.path.join(str(tmp_path), "mobilenet_wiring.pt")
    torch.save(plain_net().state_dict(), path)
    return path


def build_product(path):
    return zoo().build_classifier("mobilenet", num_classes=T.CLASSES, weights=path, device=DEV, dtype=BF16, channels_last=True,
                                  own_first_conv=True, own_depthwise=True, own_pointwise=True, head_fp32=True)


def refuse_the_library(mp):
    def refuse(name):
        def fn(*a, **k):
            raise AssertionError("library call: F.%s" % name)
        return fn
    for name in ("conv2d", "batch_norm", "linear", "adaptive_avg_pool2d", "hardtanh", "relu6"):
        mp.setattr(F, name, refuse(name))


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


def product_run(model, x, g_logits, mp):
    """Forward and input gradient of the product with the library patched to raise and the C ABI observed: the outputs
    of features[0 .. 18] (hooks, NHWC), the logits, the gradient with respect to x, the calls per entry point."""
    from dl_attack_on_imagenet_amd import _lib
    r, hooks = Run(), []
    r.outs = []
    for layer in model[0].features:
        hooks.append(layer.register_forward_hook(lambda m, a, out: r.outs.append(out.detach().permute(0, 2, 3, 1))))
    spy = Spy(lib())
    xi = x.detach().clone().requires_grad_(True)
    with mp.context() as m:
        refuse_the_library(m)
        m.setattr(_lib, "_lib", spy)
        logits = model(xi)
        (gx,) = torch.autograd.grad(logits, xi, g_logits)
    for hk in hooks:
        hk.remove()
    torch.cuda.synchronize()
    r.logits, r.grad, r.calls, r.x = logits.detach(), gx, spy.calls, xi
    return r


def first_mismatch(r, tape):
    """None, or the name of the first tensor of the product that differs from the tape's (values: +0 equals -0)."""
    if len(r.outs) != len(tape.outs):
        return "number of feature outputs"
    for i, (a, b) in enumerate(zip(r.outs, tape.outs)):
        if a.shape != b.shape or a.dtype != b.dtype or not torch.equal(a, b):
            return "output of features[%d]" % i
    if r.logits.shape != tape.logits.shape or r.logits.dtype != tape.logits.dtype or not torch.equal(r.logits, tape.logits):
        return "logits"
    if r.grad.shape != tape.grad.shape or r.grad.dtype != tape.grad.dtype or not torch.equal(r.grad, tape.grad):
        return IMAGE_GRADIENT
    return None


def assert_run_premises(model, r, x):
    """The run exercised what it was meant to: the rewritten modules, the ten joins, every kernel path."""
    z = zoo()
    net = model[0]
    count = lambda kind: sum(isinstance(m, kind) for m in net.modules())
    assert len(model) == 1 and isinstance(net, z.MobileNetV2) and net.head32_on and isinstance(net.head32, z._OwnHead)
    assert (count(z._OwnFirstConv), count(z._OwnDepthwise), count(z._OwnPointwise), count(z._OwnInvertedResidual)) == (1, 17, 17, 17)
    blocks = list(net.features)[1:-1]
    assert all(isinstance(b, z._OwnInvertedResidual) for b in blocks)
    assert [i for i, b in enumerate(blocks) if b.use_res] == T.RES_BLOCKS
    assert r.calls == COUNTS, r.calls
    assert len(r.outs) == 19
    for i, t in enumerate(r.outs):
        assert t.dtype == BF16 and not bool((R.bits(t) == -32768).any()), "the output of features[%d] holds -0.0" % i
    assert r.logits.dtype == F32 and r.logits.shape == (x.shape[0], T.CLASSES)
    assert r.grad.dtype == x.dtype and r.grad.shape == x.shape and r.grad.is_contiguous()
    assert bool(torch.isfinite(r.grad.float()).all()) and all(float(r.grad[:, c].float().abs().max()) > 0 for c in range(3))


# ------------------------------------------------------------------------------------- (a) the product and the tape
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32_image", "bf16_image"])
@pytest.mark.parametrize("shape", T.SHAPES, ids=["3x72x40", "1x33x17"])
def test_mobilenet_equals_the_tape_bitwise(shape, dtype, tmp_path, monkeypatch):
    t0 = time.time()
    tape = shared_tape(shape, dtype)
    shares = T.assert_premises(tape, "C-ABI tape %s" % (shape,))
    if dtype == F32:
        print("\n".join(f"{shape} ReLU6 layer {i:2d} [{a.shape[1]:2d} x {a.shape[2]:2d} x {a.shape[3]:4d}]: at 0 {s[0]:.4f}, inside "
                        f"{s[1]:.4f}, at 6 {s[2]:.5f}" for i, (a, s) in enumerate(zip(tape.acts, shares))))
    model = build_product(checkpoint(tmp_path))
    x, g = inputs(shape, dtype)
    r = product_run(model, x.to(DEV), g.to(DEV), monkeypatch)
    assert_run_premises(model, r, x)
    bad = first_mismatch(r, tape)
    assert bad is None, f"{shape} {dtype}: the product and the C-ABI tape differ first at the {bad}"
    print(f"{shape} {dtype}: 19 feature outputs, the logits and the image gradient equal the tape's; {time.time() - t0:.2f} s")


# --------------------------------------------------------------------------- (b) the tape's steps are the restatements
@pytest.mark.parametrize("shape,dtype", [(T.SHAPES[0], F32), (T.SHAPES[1], BF16)], ids=["3x72x40_fp32", "1x33x17_bf16"])
def test_every_tape_step_is_within_the_bound_of_its_restatement(shape, dtype):
    t0 = time.time()
    reference_tape(shape, dtype)
    tape, be = abi_tape(shape, dtype, keep_log=True)
    worst, count = T.step_ratios(be.log)
    for name in T.STEPS:
        print(f"{shape}: {name:10s} {count.get(name, 0):3d} steps, worst max err / bound = {worst.get(name, float('nan')):.3f}")
    assert count == {"first_fwd": 1, "first_bwd": 1, "dw_fwd": 17, "dw_bwd": 17, "pw8_fwd": 34, "pw8_bwd": 34, "head_fwd": 1,
                     "head_bwd": 1}
    for name, q in worst.items():
        assert q <= 1.0, f"{shape}: a {name} step is {q:.3f} times its bound away from the restatement"
    print(f"{shape}: {time.time() - t0:.2f} s")


# ------------------------------------------------------------------------------------------- (c) the learner's route
def test_the_learners_route_equals_the_tape_bitwise(tmp_path, monkeypatch):
    """engine.input_gradient(model, x, labels, "ce", ...) against the tape driven with the loss gradient torch computes
    from the tape's OWN logits; then inside classifier_batch_bucket(4): 3 rows padded to 4 with a zero image."""
    from dl_attack_on_imagenet_amd import engine
    t0 = time.time()
    shape = T.SHAPES[0]
    model = build_product(checkpoint(tmp_path))
    x, _ = inputs(shape, F32)
    x = x.to(DEV)
    labels = torch.tensor([3, 0, 7], device=DEV)
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
        with engine.classifier_batch_bucket(4):
            out4, ls4, gx4 = engine.input_gradient(model, x, labels, *loss)
    torch.cuda.synchronize()
    for o, g in ((out, gx), (out4, gx4)):
        assert o.dtype == F32 and o.shape == (3, T.CLASSES) and g.dtype == F32 and g.shape == x.shape and g.is_contiguous()
    assert torch.equal(out, tape.logits), "the learner's logits differ from the tape's"
    assert torch.equal(gx, tape.grad), "the learner's image gradient differs from the tape's"
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    assert torch.equal(out4, out) and torch.equal(ls4, ls), "padding the batch to 4 rows changes the logits of the real rows"
    assert torch.equal(gx4, gx), "padding the batch to 4 rows changes the image gradient of the real rows"
    print(f"learner's route: logits and image gradient equal the tape's, with and without the batch bucket; {time.time() - t0:.2f} s")


# ------------------------------------------------------------------------------------- (d) tables survive the cast
def test_tables_survive_the_casts(tmp_path, monkeypatch):
    z = zoo()
    t0 = time.time()
    model = build_product(checkpoint(tmp_path))
    model = model.to(BF16).to(memory_format=torch.channels_last)
    model = model.float().bfloat16()
    net, t = model[0], tables("cpu")
    same32 = lambda a, b: a.dtype == F32 and b.dtype == F32 and a.shape == b.shape and torch.equal(
        a.cpu().contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    seen = 0
    for m in net.modules():
        if isinstance(m, z._KeepsFp32):
            for n in m._KEEP_FP32:
                assert getattr(m, n).dtype == F32 and getattr(m, n).is_cuda, (type(m).__name__, n)
                seen += 1
    assert seen == 2 + 17 * 2 + 17 * 2 + 17 * 2 + 3
    feats = list(net.features)

    def pointwise(mod, conv, want, what):
        assert same32(mod.scale, want["scale"]) and same32(mod.shift, want["shift"]), what
        w2d = conv.weight.detach().reshape(mod.cout, mod.cin)
        assert w2d.dtype == BF16 and torch.equal(R.bits(w2d.cpu()), R.bits(want["w"])), what
        assert mod.wt2d.dtype == BF16 and mod.wt2d.is_contiguous() and torch.equal(R.bits(mod.wt2d), R.bits(w2d.t())), what

    first = feats[0]
    assert same32(first.scale, t["first"]["scale"]) and same32(first.shift, t["first"]["shift"])
    assert torch.equal(R.bits(first[0].weight.detach().cpu()), R.bits(t["first"]["w"]))
    from dl_attack_on_imagenet_amd import ops
    wf, wb = ops.pack_first3x3_weights(first[0].weight.detach())
    assert first.w_fwd.dtype == BF16 and torch.equal(R.bits(first.w_fwd), R.bits(wf)) and torch.equal(R.bits(first.w_bwd), R.bits(wb))
    assert tuple(first.mean) == t["mean"] and tuple(first.inv_std) == t["inv_std"]
    for i, (blk, want) in enumerate(zip(feats[1:-1], t["blocks"])):
        layers = list(blk.conv)
        assert (len(layers) == 4) == (want["expand"] is not None) and blk.use_res == want["use_res"]
        if want["expand"] is not None:
            pointwise(layers[0], layers[0][0], want["expand"], "expansion of block %d" % i)
        dw = layers[-3]
        assert isinstance(dw, z._OwnDepthwise) and dw.stride == want["dw"]["stride"]
        assert same32(dw.w9c, want["dw"]["w9c"]) and same32(dw.bias, want["dw"]["bias"]), "depthwise tables of block %d" % i
        pointwise(blk, layers[-2], want["proj"], "projection of block %d" % i)
    pointwise(feats[-1], feats[-1][0], t["last"], "last 1x1 layer")
    head = net.head32
    assert same32(head.weight, t["head"]["w"]) and same32(head.bias, t["head"]["bias"])
    assert same32(head.wt, t["head"]["w"].t().contiguous())
    # ... and the module that went through the casts is still the tape's function
    shape = T.SHAPES[1]
    x, g = inputs(shape, BF16)
    r = product_run(model, x.to(DEV), g.to(DEV), monkeypatch)
    assert_run_premises(model, r, x)
    assert first_mismatch(r, shared_tape(shape, BF16)) is None
    print(f"tables after the casts: {seen} fp32 buffers and 35 transposed weights hold their bits; {time.time() - t0:.2f} s")


# ------------------------------------------------------------------------------------------ (e) the comparison notices
def _mutate(mp, which, model):
    """One mutant of the product; returns the tensor that (a) must name."""
    from dl_attack_on_imagenet_amd import ops
    z = zoo()
    if which == "residual_gradient_dropped":                            # at the third join from the end (block 12) only
        real, seen = ops.Pointwise8Function.backward, [0]

        def backward(ctx, g):
            out = real(ctx, g)
            if ctx.meta[3]:
                seen[0] += 1
                if seen[0] == 3:
                    assert out[5] is not None
                    return out[:5] + (None,) + out[6:]
            return out
        mp.setattr(ops.Pointwise8Function, "backward", staticmethod(backward))
        return IMAGE_GRADIENT
    if which == "depthwise_mask_ignored":                               # the fifth depthwise gradient call (block 12) only
        real, seen = ops.DepthwiseConv3x3Function.backward, [0]

        def backward(ctx, g):
            seen[0] += 1
            if seen[0] == 5:
                h, w, stride, relu6 = ctx.meta
                assert relu6 == 1
                ctx.meta = (h, w, stride, 0)
            return real(ctx, g)
        mp.setattr(ops.DepthwiseConv3x3Function, "backward", staticmethod(backward))
        return IMAGE_GRADIENT
    if which == "residual_dropped":      # no non-residual block has input and output of one shape: `res` dropped on block 4
        real, target = z._OwnInvertedResidual.forward, model[0].features[5]
        assert target.use_res

        def forward(self, x):
            if self is not target:
                return real(self, x)
            self.use_res = False
            try:
                return real(self, x)
            finally:
                self.use_res = True
        mp.setattr(z._OwnInvertedResidual, "forward", forward)
        return "output of features[5]"
    raise KeyError(which)


MUTANTS = ["residual_gradient_dropped", "depthwise_mask_ignored", "residual_dropped"]


@pytest.mark.parametrize("which", MUTANTS)
def test_a_mutant_of_the_product_is_reported(which, tmp_path, monkeypatch):
    t0 = time.time()
    shape = T.SHAPES[0]
    tape = shared_tape(shape, F32)
    model = build_product(checkpoint(tmp_path))
    x, g = inputs(shape, F32)
    with monkeypatch.context() as mp:
        expect = _mutate(mp, which, model)
        r = product_run(model, x.to(DEV), g.to(DEV), mp)
    assert r.calls == COUNTS                                            # every call is still made: only an operand is missing
    bad = first_mismatch(r, tape)
    print(f"mutant {which}: first mismatch at the {bad}; {time.time() - t0:.2f} s")
    assert bad == expect, (bad, expect)
    r = product_run(model, x.to(DEV), g.to(DEV), monkeypatch)           # ... and the sound product is back
    assert first_mismatch(r, tape) is None


def test_what_the_loose_recipe_makes_of_the_mutants(tmp_path, monkeypatch):
    """For the record (printed, not asserted): the recipe of test_mobilenet_on_own_pointwise_kernels and its three siblings
    (the input gradient of sum logits^2 no further from the fp32 network's than 1.5 x the plain bf16 network's, relative)
    on this network and the 3 x 3 x 72 x 40 batch, for the sound product and for the three mutants.  Measured on the MI355X:
    see profiles/mobilenet_wiring.md."""
    t0 = time.time()
    path = checkpoint(tmp_path)
    kw = dict(num_classes=T.CLASSES, weights=path, device=DEV)
    ref = zoo().build_classifier("mobilenet", **kw)
    off = zoo().build_classifier("mobilenet", dtype=BF16, channels_last=True, **kw)
    own = build_product(path)
    x = inputs(T.SHAPES[0], F32)[0].to(DEV)

    def gradient(m, xi):
        xi = xi.clone().requires_grad_(True)
        return torch.autograd.grad(m(xi).float().square().sum(), xi)[0].float()

    gr = gradient(ref, x)
    rel = lambda g: float((g - gr).norm() / gr.norm())
    r0 = rel(gradient(off, x.bfloat16()))
    print(f"loose recipe: plain bf16 network {r0:.4f}, so the margin is {1.5 * r0:.4f}")
    for which in [None] + MUTANTS:
        with monkeypatch.context() as mp:
            if which:
                _mutate(mp, which, own)
            g1 = gradient(own, x.bfloat16())
        assert bool(torch.isfinite(g1).all())
        print(f"loose recipe, {which or 'sound product'}: relative error {rel(g1):.4f} ({'inside' if rel(g1) <= 1.5 * r0 else 'outside'} "
              f"the margin)")
    print(f"loose recipe: {time.time() - t0:.2f} s")


# ------------------------------------------------------------------------------------------------- (f) two fresh builds
def test_two_fresh_builds_agree_bitwise(tmp_path, monkeypatch):
    t0 = time.time()
    shape = T.SHAPES[0]
    path = checkpoint(tmp_path)
    x, g = inputs(shape, F32)
    a = product_run(build_product(path), x.to(DEV), g.to(DEV), monkeypatch)
    b = product_run(build_product(path), x.to(DEV), g.to(DEV), monkeypatch)
    bits32 = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits32(a.logits), bits32(b.logits)) and torch.equal(bits32(a.grad), bits32(b.grad))
    for t, u in zip(a.outs, b.outs):
        assert torch.equal(R.bits(t), R.bits(u))
    print(f"two fresh builds: logits, image gradient and 19 feature outputs hold the same bits; {time.time() - t0:.2f} s")
