"""Proves tests/mobilenet_tape.py, on the CPU: the tape over the restatements with every rounding taken out
(classifier_reference.Unrounded) is a plain fp64 function, and must be the function of the torch modules (zoo.Normalize +
zoo.MobileNetV2, eval mode, fp64, autograd) on the same weights, image and logit gradient: the 19 outputs of features[0 ..
18], the logits and the gradient with respect to the image, on both image shapes.

Bound.  Both sides evaluate the same real function in fp64 with different summation orders (and (x - m) * (1 / s) for
(x - m) / s, x * (w s) + (b - m s) for ((x * w) - m) * s' + b: a few roundings more per layer).  One output of one layer is
a sum of n <= 1280 + 3 terms, so its two evaluations differ by at most 2 n 2^-53 sum|terms|; sum|terms| / |result| is a few
tens for these random weights, and the differences add up over 53 layers each way: about 2 * 1283 * 2^-53 * 50 * 106 = 1.5e-9
relative to the largest value in the WORST case, and by the usual square-root law about 1e-13 in practice.  The tests
assert max|diff| <= 1e-9 max|ref| per tensor (the bound of the ResNet proof) and print the observed ratio.  A wiring mistake
moves the result by order 1: every mutant of the tape must fail the very same comparison, at the tensor named for it.

The restatements form three fp32 products by definition (the normalised pixel, bf16(g * scale), pooled = S * f32(1 / HW));
over `Unrounded` alone they are the real products (`ar.f32`, head_reference.scale_f32)."""
import pytest
import torch

import classifier_reference as R
import mobilenet_tape as T

BOUND = 1e-9
IMAGE_GRADIENT = "gradient with respect to the image"

_NET, _CACHE = [], {}


def net64():
    if not _NET:
        net = T.make_net()
        _NET.extend([net, T.layer_tables(net)])
    return _NET


def plain(shape):
    """(tables, x, g, the 19 feature outputs NHWC, logits, image gradient) of the plain fp64 network; once per shape."""
    if shape not in _CACHE:
        from dl_attack_on_imagenet_amd import zoo
        net, tables = net64()
        model = torch.nn.Sequential(zoo.Normalize(T.MEAN, T.STD), net).double().eval()
        x, g = T.make_inputs(shape)
        xi = x.double().requires_grad_(True)
        feats, h = [], model[0](xi)
        for layer in model[1].features:
            h = layer(h)
            feats.append(h.detach().permute(0, 2, 3, 1).clone())       # before the next layer's in-place ReLU6 can touch it
            h = h + 0.0
        logits = model[1].classifier(torch.flatten(torch.nn.functional.adaptive_avg_pool2d(h, 1), 1))
        assert torch.equal(logits.detach(), model(x.double()))
        (gx,) = torch.autograd.grad(logits, xi, g.double())
        net.float()
        _CACHE[shape] = (tables, x, g, feats, logits.detach(), gx.contiguous())
    return _CACHE[shape]


def names():
    return ["output of features[%d]" % i for i in range(19)] + ["logits", IMAGE_GRADIENT]


def ratios(tape, feats, logits, gx):
    """max|diff| / max|ref| of the 19 feature outputs, the logits and the image gradient, in that order."""
    out = []
    for a, b in zip(tape.outs + [tape.logits, tape.grad], feats + [logits, gx]):
        assert a.shape == b.shape, (a.shape, b.shape)
        q = float((a - b).abs().max() / b.abs().max())
        out.append(q if q == q else float("inf"))
    return out


def first_mismatch(qs):
    return next((n for n, q in zip(names(), qs) if not q <= BOUND), None)


@pytest.mark.parametrize("shape", T.SHAPES)
def test_unrounded_tape_is_the_plain_network(shape):
    tables, x, g, feats, logits, gx = plain(shape)
    be = T.Restate(R.Unrounded())
    tape = T.run_tape(be, tables, x, g)
    assert len(tape.outs) == len(feats) == 19 and be.steps == 2 * (1 + 17 + 34 + 1)
    shares = T.assert_premises(tape, str(shape))                       # on the reference alone
    assert not bool((gx == 0).any()), "the image gradient has zero elements"
    qs = ratios(tape, feats, logits, gx)
    rms = [float(gx[:, c].square().mean().sqrt()) for c in range(3)]
    print(f"{shape}: {be.steps} steps, worst max|diff| / max|ref| = {max(qs):.3e} at the {names()[qs.index(max(qs))]}; "
          f"image gradient rms per channel {rms[0]:.3g} {rms[1]:.3g} {rms[2]:.3g}; ReLU6 shares at 0: "
          f"{min(s[0] for s in shares):.3f} .. {max(s[0] for s in shares):.3f}, at 6 (from the second layer): "
          f"{min(s[2] for s in shares[1:]):.5f} .. {max(s[2] for s in shares[1:]):.5f}")
    assert first_mismatch(qs) is None and max(qs) <= BOUND, (first_mismatch(qs), max(qs))


def test_table_recipes_of_the_product_are_the_fp64_ones_rounded_once():
    """What the GPU leg feeds the tape.  zoo._bn_affine: the scale is the fp64 scale rounded once to fp32; the shift uses the
    ROUNDED scale (as the kernels apply it), so it is within one fp32 step of |mean| |scale| + |shift| of the fp64 one.  The
    depthwise tables: w * scale64 and beta - mean * scale64, each formed in fp64 and rounded once: the fp64 tables' `.float()`,
    bit for bit.  Weights: the fp64 ones (bf16 values) unchanged; the head: the Linear's own fp32 bits."""
    from dl_attack_on_imagenet_amd import zoo
    net, t64 = net64()
    t32 = T.layer_tables(net, product=True)
    pairs = [(t64["first"], t32["first"]), (t64["last"], t32["last"])]
    for a, b in zip(t64["blocks"], t32["blocks"]):
        assert a["use_res"] == b["use_res"] and a["dw"]["stride"] == b["dw"]["stride"] and (a["expand"] is None) == (b["expand"] is None)
        pairs += [(a["proj"], b["proj"])] + ([(a["expand"], b["expand"])] if a["expand"] is not None else [])
        assert b["dw"]["w9c"].dtype == b["dw"]["bias"].dtype == torch.float32
        assert torch.equal(b["dw"]["w9c"], a["dw"]["w9c"].float()) and torch.equal(b["dw"]["bias"], a["dw"]["bias"].float())
    assert len(pairs) == 35
    bns = [m for m in net.features.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 52
    for m in bns:
        s32, b32 = zoo._bn_affine(m)
        s64, b64 = T.bn_affine64(m)
        assert s32.dtype == b32.dtype == torch.float32 and torch.equal(s32, s64.float())
        assert bool(((b32.double() - b64).abs() <= 2.0 ** -23 * (b64.abs() + m.running_mean.double().abs() * s64.abs())).all())
    for a, b in pairs:
        assert b["w"].dtype == torch.bfloat16 and torch.equal(b["w"].double(), a["w"])
        assert b["scale"].dtype == torch.float32 and torch.equal(b["scale"], a["scale"].float())
    assert torch.equal(t32["head"]["w"].double(), t64["head"]["w"]) and t32["head"]["w"].dtype == torch.float32
    f32 = lambda v: torch.tensor(v, dtype=torch.float64).float()
    assert torch.equal(f32(t32["mean"]), f32(t64["mean"]))             # the same fp32 arguments; 1 / std within an fp32 step
    assert bool(((f32(t32["inv_std"]).double() - torch.tensor(t64["inv_std"])).abs() <= 2.0 ** -23 * torch.tensor(t64["inv_std"])).all())
    assert [i for i, b in enumerate(t32["blocks"]) if b["use_res"]] == T.RES_BLOCKS
    assert [i for i, b in enumerate(t32["blocks"]) if b["dw"]["stride"] == 2] == T.S2_BLOCKS


# (mutant, block index 0 .. 16 = features[1 + index], the first tensor that must differ)
MUTANTS = [
    ("drop_res_fwd", 2, "output of features[3]"),        # the residual dropped in one block's forward
    ("drop_res_fwd", 15, "output of features[16]"),
    ("drop_res_grad", 4, IMAGE_GRADIENT),                # the residual gradient dropped at one join
    ("drop_res_grad", 15, IMAGE_GRADIENT),
    ("drop_res_grad_all", -1, IMAGE_GRADIENT),           # ... at all ten joins
    ("dw_no_mask", 0, IMAGE_GRADIENT),                   # the ReLU6 mask of one depthwise backward omitted
    ("dw_no_mask", 13, IMAGE_GRADIENT),
    ("expand_mask_from_proj", 8, IMAGE_GRADIENT),        # the mask of one expansion backward from the projection's output
    ("res_on_plain", 0, "output of features[1]"),        # the projection of one non-residual block given `res`
    ("swap_scale_bwd", 11, IMAGE_GRADIENT),              # expansion and projection `scale` swapped in one block's backward
    ("s2_as_s1", 1, IMAGE_GRADIENT),                     # one stride-2 gradient scattered as stride 1 on the sub-grid
    ("s2_as_s1", 6, IMAGE_GRADIENT),
]


@pytest.mark.parametrize("shape", T.SHAPES)
@pytest.mark.parametrize("name,block,expect", MUTANTS)
def test_every_tape_mutant_fails_the_comparison(name, block, expect, shape):
    tables, x, g, feats, logits, gx = plain(shape)
    tape = T.run_tape(T.Restate(R.Unrounded()), tables, x, g, mut=(name, block))
    qs = ratios(tape, feats, logits, gx)
    bad = first_mismatch(qs)
    print(f"{shape} mutant {name} at block {block}: first mismatch at the {bad}, max|diff| / max|ref| there "
          f"{qs[names().index(bad)] if bad else 0.0:.3e}")
    assert bad is not None, f"the mutant {name} at block {block} passes the comparison"
    assert bad == expect, (bad, expect)
    assert not qs[names().index(bad)] <= 1e-4, f"the mutant {name} at block {block} moves the {bad} by {qs[names().index(bad)]:.3e} only"


def test_rounded_tape_runs_on_both_arithmetics():
    """The tape with the kernels' roundings, once over the fp64 reference arithmetic and once over its fp32-chunked
    emulation of a kernel, on the product's tables: the same tape code drives both.  Shapes and finiteness only; the
    distance is printed (the network is chaotic in bf16: it serves no precision comparison)."""
    net, _ = net64()
    t32 = T.layer_tables(net, product=True)
    for shape in T.SHAPES:
        tables, x, g, feats, logits, gx = plain(shape)
        a = T.run_tape(T.Restate(R.Arith()), t32, x, g)
        b = T.run_tape(T.Restate(R.Arith(R.F32, 16)), t32, x, g)
        for t, u, ref in zip(a.outs + [a.logits, a.grad], b.outs + [b.logits, b.grad], feats + [logits, gx]):
            assert t.shape == u.shape == ref.shape and bool(torch.isfinite(t).all()) and bool(torch.isfinite(u).all())
        for t in a.outs + b.outs:
            assert torch.equal(t, R.bf16_rne(t))                       # bf16 values throughout
        for t in (a.logits, a.grad, b.logits, b.grad):
            assert torch.equal(t.double(), t.double().float().double())   # fp32 values: the logits and an fp32 image's gradient
        rel = lambda p, q: float((p.double() - q.double()).norm() / q.double().norm())
        print(f"{shape} rounded tape: logits fp64-rounded vs emulation {rel(b.logits, a.logits):.3e}, vs unrounded "
              f"{rel(a.logits, logits):.3e}; image gradient {rel(b.grad, a.grad):.3e}, vs unrounded {rel(a.grad, gx):.3e}")
