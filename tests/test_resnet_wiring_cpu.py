"""Proves tests/resnet_tape.py, on the CPU: the tape over the restatements with every rounding taken out
(classifier_reference.Unrounded) is a plain fp64 function, and must be the function of the torch modules of zoo.ResNet
(layer1 .. layer4, eval mode, fp64, autograd) on the same weights, p and g: every block output and the gradient with
respect to p.

Bound.  Both sides evaluate the same real function in fp64 with different summation orders.  One output of one layer is
a sum of n <= 9 * 512 + 3 terms, so its two evaluations differ by at most 2 n 2^-53 sum|terms|; sum|terms| / |result| is
a few tens for these random weights, and the differences add up over at most 18 layers each way: about
2 * 4611 * 2^-53 * 50 * 36 = 2e-9 relative to the largest value in the WORST case, and by the usual square-root law about
1e-13 in practice.  The tests assert max|diff| <= 1e-9 max|ref| and print the observed ratio (1e-15 .. 1e-14).  A wiring
mistake moves the result by order 1: every mutant of the tape must fail the very same comparison, and does."""
import pytest
import torch

import classifier_reference as R
import resnet_tape as T

BOUND = 1e-9


def _nchw(t):
    return t.permute(0, 3, 1, 2)


_CACHE = {}


def plain(kind):
    """(tables, p, g, block outputs NHWC, gradient NHWC) of the plain fp64 network; computed once per network."""
    if kind not in _CACHE:
        net = T.make_net(kind).double()
        p, g = (t.double() for t in T.make_inputs(kind))
        x = _nchw(p).clone().requires_grad_(True)
        outs, h = [], x
        for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
            for blk in layer:
                h = blk(h)
                outs.append(h.detach().permute(0, 2, 3, 1).clone())
        (gp,) = torch.autograd.grad(h, x, _nchw(g))
        tables = T.layer_tables(net, T.bn_affine64)
        _CACHE[kind] = (tables, p, g, outs, gp.permute(0, 2, 3, 1).contiguous())
    return _CACHE[kind]


def worst_ratio(tape, outs, gp):
    """max over the block outputs and the gradient of max|diff| / max|ref|, and where it is."""
    worst, where = 0.0, None
    for i, (a, b) in enumerate(zip(tape.outs + [tape.grad], outs + [gp])):
        assert a.shape == b.shape, (i, a.shape, b.shape)
        q = float((a - b).abs().max() / b.abs().max())
        if not q <= worst:                                             # a NaN counts as the worst
            worst, where = q, ("block %d" % i if i < len(outs) else "gradient")
    return worst, where


@pytest.mark.parametrize("kind,joins", [("bottleneck", True), ("bottleneck", False), ("basic", False)])
def test_unrounded_tape_is_the_plain_network(kind, joins):
    tables, p, g, outs, gp = plain(kind)
    be = T.Restate(R.Unrounded())
    tape = T.run_tape(be, tables, p, g, joins=joins)
    assert len(tape.outs) == len(outs) and float(gp.abs().max()) > 0 and float(outs[-1].abs().max()) > 0
    q, where = worst_ratio(tape, outs, gp)
    print(f"{kind} joins={joins}: {be.steps} steps, worst max|diff| / max|ref| = {q:.3e} at {where}; "
          f"max|out| = {float(outs[-1].abs().max()):.3g}, max|grad| = {float(gp.abs().max()):.3g}")
    assert q <= BOUND, (q, where)


def test_table_recipe_of_the_product_is_the_fp64_one_rounded():
    """zoo._bn_affine, which the GPU leg feeds the tape: its scale is the fp64 scale rounded once to fp32; its shift uses the
    ROUNDED scale (as the kernels apply it), so it is within one fp32 step of |mean| |scale| + |shift| of the fp64 one."""
    from dl_attack_on_imagenet_amd import zoo
    net = T.make_net("basic")
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            s32, b32 = zoo._bn_affine(m)
            s64, b64 = T.bn_affine64(m)
            assert s32.dtype == b32.dtype == torch.float32 and torch.equal(s32, s64.float())
            assert bool(((b32.double() - b64).abs() <= 2.0 ** -23 * (b64.abs() + m.running_mean.double().abs() * s64.abs())).all())


# (network, joins, mutant, block index): block indices are positions in layer1 + layer2 + layer3 + layer4
#   bottleneck [3, 2, 2, 1]: 0 1 2 | 3 4 | 5 6 | 7;   basic [2, 2, 1, 1]: 0 1 | 2 3 | 4 | 5
MUTANTS = [
    ("bottleneck", True, "drop_g2", 3),          # g2 dropped at one block (the twin gradient of layer2's first block)
    ("bottleneck", False, "drop_g2", 1),
    ("bottleneck", True, "drop_g3", 2),          # g3 dropped at one stage boundary
    ("bottleneck", True, "drop_g3", 6),
    ("bottleneck", True, "g3_transposed", 2),    # g3 placed with sub_w = OH instead of OW
    ("bottleneck", True, "g3_transposed", 4),
    ("basic", True, "res_from_main", 1),         # the residual taken from the main-path tensor
    ("bottleneck", True, "mask_neighbour", 4),   # the ReLU mask y of the neighbouring block
    ("bottleneck", False, "mask_neighbour", 1),
    ("basic", True, "mask_neighbour", 1),
    ("bottleneck", True, "pre_bn1", 1),          # the prologue tables of bn1 instead of bn2 (inside a join)
    ("bottleneck", True, "pre_bn1", 6),          # ... and in a plain pointwise call
    ("bottleneck", True, "gather_odd_row", 3),   # the stride-2 gather reading pixel (2oh+1, 2ow)
    ("basic", True, "gather_odd_row", 2),
    ("bottleneck", True, "join_swap", 1),        # the join's g_out handed on in place of its gres
]


@pytest.mark.parametrize("kind,joins,name,block", MUTANTS)
def test_every_tape_mutant_fails_the_comparison(kind, joins, name, block):
    tables, p, g, outs, gp = plain(kind)
    tape = T.run_tape(T.Restate(R.Unrounded()), tables, p, g, joins=joins, mut=(name, block))
    q, where = worst_ratio(tape, outs, gp)
    print(f"{kind} joins={joins} mutant {name} at block {block}: worst max|diff| / max|ref| = {q:.3e} at {where}")
    assert not q <= BOUND, f"the mutant {name} at block {block} passes the comparison ({q:.3e})"
    assert not q <= 1e-4, f"the mutant {name} at block {block} moves the result by {q:.3e} only"


def test_rounded_tape_runs_on_both_arithmetics():
    """The tape with the kernels' roundings, once over the fp64 reference arithmetic and once over its fp32-chunked
    emulation of a kernel: the same tape code drives both.  Shapes and finiteness only; the distance is printed."""
    tables, p, g, outs, gp = plain("bottleneck")
    a = T.run_tape(T.Restate(R.Arith()), tables, p, g)
    b = T.run_tape(T.Restate(R.Arith(R.F32, 16)), tables, p, g)
    for t, u, ref in zip(a.outs + [a.grad], b.outs + [b.grad], outs + [gp]):
        assert t.shape == u.shape == ref.shape and bool(torch.isfinite(t).all()) and bool(torch.isfinite(u).all())
        assert torch.equal(t, R.bf16_rne(t)) and torch.equal(u, R.bf16_rne(u))       # bf16 values throughout
    rel = lambda x, y: float((x.double() - y.double()).abs().max() / y.abs().max())
    print(f"rounded tape: output fp64-rounded vs emulation {rel(b.outs[-1], a.outs[-1]):.3e}, vs unrounded "
          f"{rel(a.outs[-1], outs[-1]):.3e}; gradient {rel(b.grad, a.grad):.3e}, vs unrounded {rel(a.grad, gp):.3e}")
