"""CPU: host side of the narrow-channel pointwise kernels (adil_pw8_fwd / adil_pw8_bwd): the built library exports the
symbols and the header declares them, the fp64 restatement of tests/pointwise8_reference.py against torch's convolution,
BatchNorm, hardtanh and autograd, the fp32 emulation of the kernel on both legs for every row of the GPU table, the
vacuity assertions of the exact leg on the reference alone, the exact leg's power to reject mutants, the `own_pointwise`
switch and the CLI default."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import pointwise8_reference as pref
from classifier_reference import BF16, F32, Arith

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"adil_pw8_fwd": 11, "adil_pw8_bwd": 10}


def test_library_exports_and_header_declares_the_new_symbols():
    from dl_attack_on_imagenet_amd import _lib
    from dl_attack_on_imagenet_amd.build import build_library
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIBPATH)
    src = open(os.path.join(ROOT, "include", "adil_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    bound = _lib.load()
    assert bound.adil_abi_version() == _lib.ABI_VERSION == 8
    # refusals need no device: they return before any HIP call
    f, b = bound.adil_pw8_fwd, bound.adil_pw8_bwd
    assert f(None, None, None, None, None, None, 8, 8, 8, 0, None) == -1
    assert b(None, None, None, None, None, 8, 8, 8, 0, None) == -1
    for (m, k, n, act) in [(8, 12, 8, 0), (8, 8, 20, 0), (8, 2056, 8, 0), (8, 8, 2056, 1), (0, 8, 8, 0), (8, 8, 8, 2), (8, 8, 8, -1),
                           (8, 0, 8, 0), (-1, 8, 8, 1)]:
        assert f(16, 16, 16, 16, None, 16, m, k, n, act, None) == -1
        assert b(16, 16, 16, 16, 16, m, k, n, act, None) == -1
    assert f(16, 16, 16, 16, 16, 16, 8, 8, 8, 1, None) == -1            # res with act 1
    assert b(16, None, 16, 16, 16, 8, 8, 8, 1, None) == -1             # act 1 needs y
    assert f(16, 16, 16, 16, None, 24, 8, 8, 8, 0, None) == -1         # misaligned y
    assert b(8, 16, 16, 16, 16, 8, 8, 8, 0, None) == -1                # misaligned g


CASES = [(2, 5, 7, 16, 96, 1, False), (2, 5, 7, 144, 24, 0, True), (1, 1, 1, 8, 8, 1, False), (3, 4, 4, 24, 40, 0, False),
         (1, 3, 3, 320, 1280, 1, False), (2, 3, 5, 72, 136, 0, True)]


@pytest.mark.parametrize("b,h,w,k,n,act,with_res", CASES)
def test_restatement_equals_torch(b, h, w, k, n, act, with_res):
    """fp64: pw8_fwd against F.conv2d + F.batch_norm (eval) + add + hardtanh(0, 6), pw8_bwd against autograd (with scale
    values that are bf16 values and g * scale exact in bf16, so that the kernel's rounding of gz is the identity), to 1e-12."""
    from dl_attack_on_imagenet_amd import zoo
    name = "restate/%s" % ((b, h, w, k, n, act),)
    m = b * h * w
    op = pref.operands(name, "gaussian", m, k, n, with_res)
    gen = torch.Generator().manual_seed(3)
    bn = torch.nn.BatchNorm2d(n).double().eval()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(n, generator=gen))
        bn.bias.copy_(torch.randn(n, generator=gen))
        bn.running_mean.copy_(torch.randn(n, generator=gen))
        bn.running_var.copy_(torch.rand(n, generator=gen) + 0.1)
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    shift = bn.bias.detach() - bn.running_mean * scale
    s32, b32 = zoo._bn_affine(bn)
    assert s32.dtype == b32.dtype == F32 and torch.equal(s32, scale.float())
    assert torch.equal(b32, (bn.bias.detach() - bn.running_mean * s32.double()).float())      # the tables the modules hold
    ar = Arith()
    o = pref.pw8_fwd(ar, op.x, op.w, scale, shift, op.res, act)
    nchw = lambda t: t.double().reshape(b, h, w, -1).permute(0, 3, 1, 2)
    xin = nchw(op.x).clone().requires_grad_(True)
    pre = F.batch_norm(F.conv2d(xin, op.w.double().reshape(n, k, 1, 1)), bn.running_mean, bn.running_var, bn.weight, bn.bias,
                       False, 0.0, bn.eps)
    if with_res:
        pre = pre + nchw(op.res)
    yref = F.hardtanh(pre, 0.0, 6.0) if act else pre
    yr = yref.detach().permute(0, 2, 3, 1).reshape(m, n)
    got = pref.expected(o)
    assert o.n == k + 2 + int(with_res)
    assert float((got - yr).abs().max()) <= 1e-12 * max(1.0, float(yr.abs().max()))
    # gradient: scales of +-1/2, +-1, +-2 keep bf16(g * scale) == g * scale, which is what autograd multiplies by
    ex = pref.operands(name, "rounding", m, k, n)
    with torch.no_grad():
        bn.weight.copy_(ex.scale.double() * torch.sqrt(bn.running_var + bn.eps))
    xin2 = nchw(op.x).clone().requires_grad_(True)
    pre2 = F.batch_norm(F.conv2d(xin2, op.w.double().reshape(n, k, 1, 1)), bn.running_mean, bn.running_var, bn.weight, bn.bias,
                        False, 0.0, bn.eps)
    y2 = F.hardtanh(pre2, 0.0, 6.0) if act else pre2
    (gref,) = torch.autograd.grad(y2, xin2, nchw(ex.g))
    scale2 = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    ob = pref.pw8_bwd(ar, ex.g, y2.detach().permute(0, 2, 3, 1).reshape(m, n) if act else None, ex.scale, op.wt, act)
    assert float((scale2 - ex.scale.double()).abs().max()) < 1e-14 and ob.n == n
    gr = gref.permute(0, 2, 3, 1).reshape(m, k)
    assert float((ob.pre - gr).abs().max()) <= 1e-10 * max(1.0, float(gr.abs().max()))


def _legs(act):
    return ([("clamp", 1)] if act else []) + [("rounding", 0)]


def _references(row, leg, a):
    """Operands and the fp64 references of one exact-leg comparison, every premise asserted on the reference alone."""
    M, K, N, act, with_res = row
    name = "p8/%s/%s" % (row, leg)
    op = pref.operands(name, leg, M, K, N, with_res and not a)
    res = None if a else op.res
    ref = pref.pw8_fwd(Arith(), op.x, op.w, op.scale, op.shift, res, a)
    stats = [pref.assert_premise(name + "/fwd", ref, leg)]
    y = None
    if a:
        y = pref.mask_source(name, leg, pref.finish(Arith(), ref))
        stats.append(pref.assert_branches(name + "/fwd", ref.pre))
        stats.append(pref.assert_branches(name + "/mask", y.double()))
    refb = pref.pw8_bwd(Arith(), op.g, y, op.scale, op.wt, a)
    stats.append(pref.assert_premise(name + "/bwd", refb, leg))
    return name, op, res, y, ref, refb, stats


@pytest.mark.parametrize("row", pref.ROWS + [(m, k, n, 1, False) for m, k, n in pref.NAN_ROWS], ids=str)
def test_emulation_passes_both_legs_and_the_premises_hold(row):
    """Every row of the GPU table, with the kernel replaced by its fp32 emulation (chunks of 16): the vacuity assertions
    (premise, 5 % per ReLU6 branch in the pre-activation and in the gradient's mask, 10 % of the rounding set's outputs
    inexact) on the reference alone, then bit for bit on the exact legs and under the bound on the gaussian leg."""
    M, K, N, act, with_res = row
    emu = Arith(F32, chunk=16)
    for leg, a in _legs(act):
        name, op, res, y, ref, refb, stats = _references(row, leg, a)
        print(name, stats)
        pref.compare_exact(name + "/fwd", pref.finish(emu, pref.pw8_fwd(emu, op.x, op.w, op.scale, op.shift, res, a)), ref)
        pref.compare_exact(name + "/bwd", pref.finish(emu, pref.pw8_bwd(emu, op.g, y, op.scale, op.wt, a)), refb)
    name = "p8/%s/gaussian" % (row,)
    op = pref.operands(name, "gaussian", M, K, N, with_res)
    ref = pref.pw8_fwd(Arith(), op.x, op.w, op.scale, op.shift, op.res, act)
    got = pref.finish(emu, pref.pw8_fwd(emu, op.x, op.w, op.scale, op.shift, op.res, act))
    rf = pref.gaussian_ratio(got, ref)
    y = got.to(BF16) if act else None
    refb = pref.pw8_bwd(Arith(), op.g, y, op.scale, op.wt, act)
    rb = pref.gaussian_ratio(pref.finish(emu, pref.pw8_bwd(emu, op.g, y, op.scale, op.wt, act)), refb)
    print(name, "max |err| / bound: fwd %.3f bwd %.3f" % (rf, rb))
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)


MUTANT_ROWS = [(129, 24, 40, 1, False), (129, 24, 40, 0, True), (200, 16, 96, 1, False), (130, 200, 136, 1, False),
               (64, 72, 24, 0, True)]
MUTANTS = ["trunc", "ge_mask", "no_lt6", "no_clamp6", "k_tail", "n_tail", "no_scale_bwd", "no_shift", "no_res"]


def _exact_leg(emu):
    """The exact leg of tests/test_gpu_pointwise8.py with the kernel replaced by the emulation `emu`; returns the names of
    the comparisons that failed."""
    failed = []
    for row in MUTANT_ROWS:
        for leg, a in _legs(row[3]):
            name, op, res, y, ref, refb, _ = _references(row, leg, a)
            for what, o, got in (("fwd", ref, lambda: pref.finish(emu, pref.pw8_fwd(emu, op.x, op.w, op.scale, op.shift, res, a))),
                                 ("bwd", refb, lambda: pref.finish(emu, pref.pw8_bwd(emu, op.g, y, op.scale, op.wt, a)))):
                try:
                    pref.compare_exact(name + "/" + what, got(), o)
                except AssertionError:
                    failed.append(name + "/" + what)
    return failed


def test_exact_leg_passes_the_emulation_and_rejects_mutants():
    assert _exact_leg(Arith(F32, chunk=16)) == []
    for m in MUTANTS:
        failed = _exact_leg(Arith(F32, chunk=16, mut=(m,)))
        print(m, "rejected by", len(failed), "comparisons, e.g.", failed[:2])
        assert failed, "mutant %s passes the exact leg" % m


def _own(model):
    from dl_attack_on_imagenet_amd import zoo
    return [m for m in model.modules() if isinstance(m, zoo._Pw8Tables)]


def test_switch_rewrites_the_34_pointwise_layers_and_nothing_else():
    from dl_attack_on_imagenet_amd import zoo
    kw = dict(num_classes=10, seed=1, dtype=torch.bfloat16, channels_last=True)
    with pytest.raises(ValueError, match="own_pointwise"):
        zoo.build_classifier("resnet18", own_pointwise=True, **kw)
    with pytest.raises(ValueError, match="own_pointwise"):
        zoo.build_classifier("mobilenet", num_classes=10, seed=1, channels_last=True, own_pointwise=True)
    with pytest.raises(ValueError, match="own_pointwise"):
        zoo.build_classifier("mobilenet", num_classes=10, seed=1, dtype=torch.bfloat16, own_pointwise=True)
    plain = zoo.build_classifier("mobilenet", num_classes=10, seed=1)
    assert zoo.use_own_pointwise_(zoo.build_classifier("mobilenet", num_classes=10, seed=1)) == 34
    off = zoo.build_classifier("mobilenet", **kw)
    off2 = zoo.build_classifier("mobilenet", own_pointwise=False, **kw)
    on = zoo.build_classifier("mobilenet", own_pointwise=True, **kw)
    both = zoo.build_classifier("mobilenet", own_pointwise=True, own_depthwise=True, **kw)
    # switch off: the module types of the parent
    assert [type(m) for m in off.modules()] == [type(m) for m in off2.modules()] == [type(m) for m in plain.modules()]
    assert _own(off) == [] and not any(isinstance(m, zoo._OwnDepthwise) for m in on.modules())
    assert sum(isinstance(m, zoo._OwnDepthwise) for m in both.modules()) == 17
    for net in (on, both):
        mods = _own(net)
        assert len(mods) == 34
        assert sum(isinstance(m, zoo._OwnPointwise) for m in mods) == 17            # 16 expansions + the 320 -> 1280 layer
        assert sum(isinstance(m, zoo._OwnInvertedResidual) for m in mods) == 17
        assert sum(m.use_res for m in mods if isinstance(m, zoo._OwnInvertedResidual)) == 10
        assert not any(isinstance(m, zoo._InvertedResidual) for m in net.modules())
        for m in mods:
            assert m.scale.dtype == m.shift.dtype == F32 and m.scale.shape == m.shift.shape == (m.cout,)
            assert m.wt2d.dtype == BF16 and m.wt2d.shape == (m.cin, m.cout) and m.wt2d.is_contiguous()
        assert sorted(net.state_dict()) == sorted(plain.state_dict()) == sorted(off.state_dict())      # torchvision key names
        for a, b in zip(off.state_dict().values(), net.state_dict().values()):
            assert torch.equal(a, b)
        # off the GPU the rewritten network runs its original modules: the same function as the switch-off network
        x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(0)).bfloat16()
        assert torch.equal(off(x), net(x))
    # the tables: fp64-derived, fp32 whatever the cast, bit for bit; the transposed weight is the weight's own rounding
    fp = zoo.build_classifier("mobilenet", num_classes=10, seed=1)
    zoo.use_own_pointwise_(fp)
    for a, b in zip(_own(fp), _own(on)):
        conv, bn = (a[0], a[1]) if isinstance(a, zoo._OwnPointwise) else (a.conv[-2], a.conv[-1])
        scale, shift = zoo._bn_affine(bn)
        assert torch.equal(b.scale, scale) and torch.equal(b.shift, shift) and torch.equal(a.scale, scale)
        assert torch.equal(b.wt2d, conv.weight.detach().reshape(a.cout, a.cin).bfloat16().t())
    with pytest.raises(ValueError):
        zoo._OwnPointwise(zoo._ConvBNReLU6(16, 16, 3, 1, 16))
    with pytest.raises(ValueError):
        zoo._OwnPointwise(zoo._ConvBNReLU6(3, 32, 1))
    # the layer table of the reference file, from the network itself at 224 x 224
    seen = []
    probe = zoo.build_classifier("mobilenet", num_classes=10, seed=1)
    for blk in probe.modules():
        if zoo._is_pointwise_block(blk):
            blk.register_forward_hook(lambda mod, args, out: seen.append((mod[0].in_channels, mod[0].out_channels,
                                                                          args[0].shape[2], 1, False)))
        elif zoo._is_projection_block(blk):
            blk.conv[-2].register_forward_hook(lambda mod, args, out, blk=blk: seen.append(
                (mod.in_channels, mod.out_channels, args[0].shape[2], 0, blk.use_res)))
    probe(torch.zeros(1, 3, 224, 224))
    assert seen == pref.MOBILENET_LAYERS_ALL34
    assert len(pref.MOBILENET_SHAPES) == 19 and sorted(set(s[:3] for s in seen)) == sorted(s[:3] for s in pref.MOBILENET_SHAPES)
    assert sorted(set(s[0] for s in seen) | set(s[1] for s in seen)) == [16, 24, 32, 64, 96, 144, 160, 192, 320, 384, 576, 960, 1280]


def test_ops_refuse_what_the_kernels_do_not_cover():
    from dl_attack_on_imagenet_amd import ops
    x = torch.zeros(2, 16, 4, 4, dtype=BF16)
    assert not ops.pw8_conv_covers(x, 16, 96)                                       # not on a GPU
    w, wt = torch.zeros(96, 16, dtype=BF16), torch.zeros(16, 96, dtype=BF16)
    with pytest.raises(ValueError):
        ops.pw8_conv(x, w, wt, torch.zeros(96), torch.zeros(96))
    with pytest.raises(ValueError):
        ops.pw8_conv(x, torch.zeros(96, 16, 1, 1, dtype=BF16), wt, torch.zeros(96), torch.zeros(96))


def test_cli_flag_defaults_to_the_library():
    import demo_dL_attack
    p = demo_dL_attack.build_parser()
    assert p.parse_args([]).own_pointwise == 0 and p.parse_args([]).own_depthwise == 0
    a = p.parse_args(["--own-pointwise", "1"])
    assert a.own_pointwise == 1 and a.own_depthwise == 0
    assert p.parse_args(["--own-pointwise", "1", "--own-depthwise", "1"]).own_depthwise == 1
    with pytest.raises(SystemExit):
        p.parse_args(["--own-pointwise", "2"])
    from test_cabi_host import test_cli_flags_match_reference
    test_cli_flags_match_reference()
