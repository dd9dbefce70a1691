"""Proves tests/densenet_tape.py, on the CPU: the tape over the restatements with every rounding taken out
(classifier_reference.Unrounded) is a plain fp64 function, and must be the function of the torch modules (zoo.Normalize +
zoo.DenseNet, eval mode, fp64, torch.cat and autograd as they are) on the same weights, image and logit gradient: the eight
feature points (the pooled stem output, the four block outputs, the three transition outputs), the pooled features, the
logits, the gradient entering each of the eight points and the gradient with respect to the image, on both image shapes,
for a reduced network (3, 4, 2, 2) at full widths and for the real (6, 12, 24, 16).

Bound.  Both sides evaluate the same real function in fp64 with different summation orders (and (x - m) * (1 / s) for
(x - m) / s, x * scale + shift for ((x - mean) / sqrt(var + eps)) * gamma + beta, the average pool in front of the 1x1
convolution instead of behind it: a few roundings more per layer).  One output of one layer is a sum of n <= 9 * 128 terms,
so its two evaluations differ by at most 2 n 2^-53 sum|terms|, and the differences add up over 121 layers each way; by the
usual square-root law that is about 1e-13 relative to the largest value.  The tests assert max|diff| <= 1e-9 max|ref| per
tensor (the bound of the ResNet and MobileNetV2 proofs) and print the observed ratio.  A wiring mistake moves the result by
order 1: every mutant of the tape must fail the very same comparison, at the tensor named for it, by more than the floor
1e-4 of tests/test_mobilenet_wiring_cpu.py.

The restatements form their prologues and a few products in fp32 by definition (`ar.f32`, head_reference.scale_f32); over
`Unrounded` alone they are the real products.

The ReLU premise (every `mid`, every prologue of a dense layer, of a transition and of the head keeps a share of its
elements inside densenet_tape.SHARE) is asserted here, on the rounded reference tape with the product's tables, so that the
GPU tests cannot pass on a dead network."""
import os

import pytest
import torch

import classifier_reference as R
import densenet_tape as T

BOUND = 1e-9
FLOOR = 1e-4                     # what a mutant must move its tensor by: the floor of tests/test_mobilenet_wiring_cpu.py
IMAGE_GRADIENT = "gradient with respect to the image"
CONFIGS = {"reduced": T.REDUCED, "real": T.REAL}

_NETS, _CACHE = {}, {}


def net64(kind):
    if kind not in _NETS:
        net, calibrated = T.make_net(CONFIGS[kind])
        _NETS[kind] = (net, T.layer_tables(net), calibrated)
    return _NETS[kind]


def names():
    pts = T.point_names()
    return pts + ["pooled features", "logits"] + ["gradient at the " + n for n in reversed(pts)] + [IMAGE_GRADIENT]


def tensors(tape):
    """The tape's tensors in the order of `names`: forward order, then the gradients from the head back to the image."""
    return tape.points + [tape.pooled, tape.logits] + list(reversed(tape.grads)) + [tape.grad]


def plain(kind, shape):
    """(tables, x, g, the reference tensors in the order of `names`) of the plain fp64 network; once per network and shape."""
    if (kind, shape) not in _CACHE:
        from dl_attack_on_imagenet_amd import zoo
        net, tables, _ = net64(kind)
        model = torch.nn.Sequential(zoo.Normalize(T.MEAN, T.STD), net).double().eval()
        x, g = T.make_inputs(shape)
        xi = x.double().requires_grad_(True)
        pts, hooks = [], []
        f = net.features
        for m in [f.pool0] + [c for n, c in f.named_children() if n.startswith(("denseblock", "transition"))]:
            hooks.append(m.register_forward_hook(lambda mod, a, out: pts.append(out)))
        pooled = []
        hooks.append(net.classifier.register_forward_hook(lambda mod, a, out: pooled.append(a[0].detach().clone())))
        logits = model(xi)
        for hk in hooks:
            hk.remove()
        assert len(pts) == 8 and len(pooled) == 1
        grads = torch.autograd.grad(logits, [xi] + pts, g.double())
        nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
        ref = [nhwc(t) for t in pts] + [pooled[0], logits.detach()] + [nhwc(t) for t in reversed(grads[1:])] + [grads[0].contiguous()]
        net.float()
        _CACHE[(kind, shape)] = (tables, x, g, ref)
    return _CACHE[(kind, shape)]


def ratios(tape, ref):
    """max|diff| / max|ref| of every tensor of `names`, in that order."""
    out = []
    got = tensors(tape)
    assert len(got) == len(ref) == len(names())
    for a, b in zip(got, ref):
        assert a.shape == b.shape, (a.shape, b.shape)
        q = float((a - b).abs().max() / b.abs().max())
        out.append(q if q == q else float("inf"))
    return out


def first_mismatch(qs):
    return next((n for n, q in zip(names(), qs) if not q <= BOUND), None)


@pytest.mark.parametrize("shape", T.SHAPES, ids=["2x96x32", "1x94x62"])
@pytest.mark.parametrize("kind", list(CONFIGS))
def test_unrounded_tape_is_the_plain_network(kind, shape):
    tables, x, g, ref = plain(kind, shape)
    be = T.Restate(R.Unrounded())
    tape = T.run_tape(be, tables, x.double(), g.double())
    assert be.steps == sum(T.step_counts(CONFIGS[kind]).values())
    assert [len(m) for m in tape.mids] == list(CONFIGS[kind])
    for n, t in zip(names(), ref):
        assert float(t.abs().max()) > 0, f"the {n} of the plain network is zero"
    qs = ratios(tape, ref)
    gx = ref[-1]
    rms = [float(gx[:, c].square().mean().sqrt()) for c in range(3)]
    print(f"{kind} {shape}: {be.steps} steps, worst max|diff| / max|ref| = {max(qs):.3e} at the {names()[qs.index(max(qs))]}; "
          f"image gradient rms per channel {rms[0]:.3g} {rms[1]:.3g} {rms[2]:.3g}")
    assert first_mismatch(qs) is None and max(qs) <= BOUND, (first_mismatch(qs), max(qs))


@pytest.mark.parametrize("shape", T.SHAPES, ids=["2x96x32", "1x94x62"])
@pytest.mark.parametrize("kind", list(CONFIGS))
def test_every_relu_of_the_rounded_reference_tape_is_alive(kind, shape):
    """The premise of the GPU tests, on the reference alone: the tape with the kernels' roundings over the fp64 reference
    arithmetic, on the product's tables."""
    net, _, calibrated = net64(kind)
    t32 = T.layer_tables(net, product=True)
    x, g = T.make_inputs(shape)
    for dtype in (torch.float32, torch.bfloat16):
        tape = T.run_tape(T.Restate(R.Arith()), t32, x.to(dtype), g)
        shares = T.assert_premises(tape, t32, f"{kind} {shape} {dtype}")
        for t in tape.points + [m for mids in tape.mids for m in mids]:
            assert torch.equal(t, R.bf16_rne(t))                       # bf16 values throughout
        lo, hi = min(shares, key=lambda s: s[1]), max(shares, key=lambda s: s[1])
        print(f"{kind} {shape} {dtype}: statistics {'calibrated on the images' if calibrated else 'drawn around 0 / 1'}; "
              f"{len(shares)} ReLU shares, lowest {lo[1]:.4f} at the {lo[0]}, highest {hi[1]:.4f} at the {hi[0]}")


# (mutant, block or transition index, layer index, the first tensor that must differ); the indices exist in both networks
MUTANTS = [
    ("short_prefix", 1, 2, "output of denseblock2"),                        # a layer reads a prefix one growth slice too short
    ("swap_slots", 2, 0, "output of denseblock3"),                          # two neighbouring layers' output slots exchanged
    ("no_accumulate", 2, 1, "gradient at the output of transition2"),       # one layer runs with accumulate = 0
    ("no_accumulate", 0, 1, "gradient at the stem output"),
    ("first_layer_first", 1, -1, "gradient at the output of transition1"),  # a block's backward walks first layer first
    ("mask_prev_mid", 3, 1, "gradient at the output of transition3"),       # a layer's mask from the previous layer's mid
    ("tr_hw_swapped", 0, -1, "output of transition1"),                      # a transition pools with H and W exchanged
    ("norm5_twice", -1, -1, "pooled features"),                             # norm5 both in the trunk and in the head
    ("tr_grad_offset", 1, -1, "gradient at the output of transition2"),     # a transition's gradient read at offset growth
]


@pytest.mark.parametrize("shape", T.SHAPES, ids=["2x96x32", "1x94x62"])
@pytest.mark.parametrize("kind", list(CONFIGS))
@pytest.mark.parametrize("name,block,layer,expect", MUTANTS)
def test_every_tape_mutant_fails_the_comparison(name, block, layer, expect, kind, shape):
    tables, x, g, ref = plain(kind, shape)
    tape = T.run_tape(T.Restate(R.Unrounded()), tables, x.double(), g.double(), mut=(name, block, layer))
    qs = ratios(tape, ref)
    bad = first_mismatch(qs)
    moved = qs[names().index(bad)] if bad else 0.0
    print(f"{kind} {shape} mutant {name} at ({block}, {layer}): first mismatch at the {bad}, max|diff| / max|ref| there {moved:.3e}")
    assert bad is not None, f"the mutant {name} at ({block}, {layer}) passes the comparison"
    assert bad == expect, (bad, expect)
    assert not moved <= FLOOR, f"the mutant {name} at ({block}, {layer}) moves the {bad} by {moved:.3e} only"


def test_table_recipes_of_the_product_are_the_modules_own_buffers(tmp_path):
    """What the GPU leg feeds the tape, against what the product feeds its kernels: zoo.build_classifier with all six
    switches, bf16, channels_last, built on the CPU from the same checkpoint.  Every table bit for bit."""
    from dl_attack_on_imagenet_amd import zoo
    net, t64, _ = net64("real")
    t32 = T.layer_tables(net, product=True)
    path = os.path.join(str(tmp_path), "densenet_wiring.pt")
    torch.save(net.state_dict(), path)
    model = zoo.build_classifier("densenet121", num_classes=T.CLASSES, weights=path, dtype=torch.bfloat16, channels_last=True,
                                 own_dense_pointwise=True, own_dense_conv=True, own_dense_block=True, own_dense_transition=True,
                                 own_dense_stem=True, own_dense_head=True)
    assert len(model) == 1
    prod = model[0]

    def same(a, b, dtype, what):
        assert a.dtype == dtype and b.dtype == dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
        view = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(a.contiguous().view(view), b.contiguous().view(view)), what
        return 1

    F32, BF16 = torch.float32, torch.bfloat16
    seen = 0
    f = prod.features
    assert isinstance(f, zoo._OwnDenseStem) and isinstance(prod.head32, zoo._OwnDenseHead) and prod.head32_on
    s = t32["stem"]
    seen += same(f.scale, s["scale"], F32, "stem scale") + same(f.shift, s["shift"], F32, "stem shift")
    seen += same(f.w_fwd, s["w_fwd"], BF16, "stem w_fwd") + same(f.w_bwd, s["w_bwd"], BF16, "stem w_bwd")
    assert tuple(f.mean) == t32["mean"] and tuple(f.inv_std) == t32["inv_std"]
    blocks = [m for n, m in f.named_children() if n.startswith("denseblock")]
    trans = [m for n, m in f.named_children() if n.startswith("transition")]
    assert [len(b) for b in blocks] == list(T.REAL) and len(trans) == 3
    assert all(isinstance(b, zoo._OwnDenseBlock) for b in blocks) and all(isinstance(t, zoo._OwnTransition) and t.pool_first for t in trans)
    for bi, (b, layers) in enumerate(zip(blocks, t32["blocks"])):
        for li, (m, t) in enumerate(zip(b.values(), layers)):
            what = "denseblock%d layer %d " % (bi + 1, li + 1)
            for key in ("pscale", "pshift", "scale", "shift"):
                seen += same(getattr(m, key), t[key], F32, what + key)
            seen += same(m.conv1.weight.detach().reshape(m.cout, m.cin), t["w"], BF16, what + "w2d")
            seen += same(m.wt2d, t["wt"], BF16, what + "wt2d")
            seen += same(m.conv2.wp_fwd, t["wp_fwd"], BF16, what + "wp_fwd") + same(m.conv2.wp_bwd, t["wp_bwd"], BF16, what + "wp_bwd")
            seen += same(m.conv2.weight.detach(), t["w3"], BF16, what + "conv2 weight")
    for ti, (m, t) in enumerate(zip(trans, t32["trans"])):
        what = "transition%d " % (ti + 1)
        seen += same(m.pscale, t["pscale"], F32, what + "pscale") + same(m.pshift, t["pshift"], F32, what + "pshift")
        seen += same(m.conv.weight.detach().reshape(m.cout, m.cin), t["w"], BF16, what + "w2d") + same(m.wt2d, t["wt"], BF16, what + "wt2d")
        assert bool((m.scale == 1).all()) and bool((m.shift == 0).all())
    h, t = prod.head32, t32["head"]
    seen += same(h.weight, t["w"], F32, "head weight") + same(h.wt, t["wt"], F32, "head wt") + same(h.bias, t["bias"], F32, "head bias")
    seen += same(h.pscale, t["pscale"], F32, "head pscale") + same(h.pshift, t["pshift"], F32, "head pshift")
    assert seen == 4 + 58 * 9 + 3 * 4 + 5
    # ... and the product's recipe is the fp64 one rounded once: weights unchanged; zoo._bn_affine's scale is the fp64 scale's
    # `.float()`, its shift uses the ROUNDED scale (as the kernels apply it), so it is within one fp32 step of
    # |mean| |scale| + |shift| of the fp64 one
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 1 + 2 * 58 + 3 + 1
    for m in bns:
        s32, b32 = zoo._bn_affine(m)
        s64, b64 = T.bn_affine64(m)
        assert s32.dtype == b32.dtype == F32 and torch.equal(s32, s64.float())
        assert bool(((b32.double() - b64).abs() <= 2.0 ** -23 * (b64.abs() + m.running_mean.double().abs() * s64.abs())).all())
    for a, b in zip(t64["blocks"], t32["blocks"]):
        for la, lb in zip(a, b):
            assert torch.equal(lb["w"].double(), la["w"]) and torch.equal(lb["w3"].double(), la["w3"])
            assert torch.equal(lb["scale"], la["scale"].float()) and torch.equal(lb["pscale"], la["pscale"].float())
    for a, b in zip(t64["trans"], t32["trans"]):
        assert torch.equal(b["w"].double(), a["w"]) and torch.equal(b["pscale"], a["pscale"].float())
    assert torch.equal(t32["stem"]["w"].double(), t64["stem"]["w"]) and torch.equal(t32["head"]["w"].double(), t64["head"]["w"])
    print(f"table recipes: {seen} buffers of the product hold the bits of the tape's tables")
