"""CPU: host side of the pre-activated pointwise kernels (adil_dense1x1_fwd / adil_dense1x1_bwd): the built library exports
the symbols and the header declares them, the restatement of tests/dense1x1_reference.py against torch's BatchNorm, ReLU,
convolution and autograd, the fp32 emulation of the kernel on both legs for every row of the GPU table, the vacuity
assertions of the exact legs on the reference alone, the comparators' power to reject mutants, the layer list against the
network itself, the `own_dense_pointwise` switch and the CLI default."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dense1x1_reference as dref
from classifier_reference import F32, SCALES, Arith

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"adil_dense1x1_fwd": 12, "adil_dense1x1_bwd": 13}


def test_library_exports_and_header_declares_the_new_symbols():
    from dl_attack_on_imagenet_amd import _lib
    from dl_attack_on_imagenet_amd.build import build_library
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIBPATH)
    src = open(os.path.join(ROOT, "include", "adil_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    bound = _lib.load()
    assert bound.adil_abi_version() == _lib.ABI_VERSION == 8
    # refusals need no device: they return before any HIP call
    f, b = bound.adil_dense1x1_fwd, bound.adil_dense1x1_bwd
    assert f(None, None, None, None, None, None, None, 8, 8, 8, 0, None) == -1
    assert b(None, None, None, None, None, None, None, None, 8, 8, 8, 0, None) == -1
    for (m, k, n, act) in [(8, 12, 8, 0), (8, 8, 20, 0), (8, 2056, 8, 0), (8, 8, 2056, 1), (0, 8, 8, 0), (8, 8, 8, 2), (8, 8, 8, -1),
                           (8, 0, 8, 0), (-1, 8, 8, 1)]:
        assert f(16, 16, 16, 16, 16, 16, 16, m, k, n, act, None) == -1
        assert b(16, 16, 16, 16, 16, 16, 16, 16, m, k, n, act, None) == -1
    assert b(16, None, 16, 16, 16, 16, 16, 16, 8, 8, 8, 1, None) == -1     # act 1 needs y
    assert f(16, 16, 16, 16, 16, 16, 24, 8, 8, 8, 0, None) == -1           # misaligned y
    assert f(16, 18, 16, 16, 16, 16, 16, 8, 8, 8, 0, None) == -1           # misaligned pscale
    assert b(8, 16, 16, 16, 16, 16, 16, 16, 8, 8, 8, 0, None) == -1        # misaligned g
    assert b(16, 16, 16, 16, 24, 16, 16, 16, 8, 8, 8, 0, None) == -1       # misaligned xin


CASES = [(2, 5, 7, 64, 128, 1), (2, 5, 7, 256, 128, 0), (1, 1, 1, 8, 8, 1), (3, 4, 4, 24, 40, 0), (2, 3, 5, 72, 136, 1)]


@pytest.mark.parametrize("b,h,w,k,n,act", CASES)
def test_restatement_equals_torch(b, h, w, k, n, act):
    """d1_fwd against F.batch_norm (eval) + relu + F.conv2d + F.batch_norm + relu, d1_bwd against autograd, in fp64 on
    operands for which the kernel's two inner roundings are the identity (integer x, pscale / scale from SCALES, integer
    pshift: pre and g * scale are bf16 values), to 1e-12; the tables are `zoo._bn_affine`'s."""
    from dl_attack_on_imagenet_amd import zoo
    gen = torch.Generator().manual_seed(3)
    m = b * h * w
    op = dref.operands("restate/%s" % ((b, h, w, k, n, act),), "gaussian", m, k, n)
    pick = lambda c: torch.tensor(SCALES, dtype=torch.float64)[torch.randint(0, len(SCALES), (c,), generator=gen)]
    x = torch.randint(-8, 9, (m, k), generator=gen).double()
    g = torch.randint(-8, 9, (m, n), generator=gen).double()

    def bn_of(c, scale, shift):                                 # a BatchNorm whose affine map is (scale, shift) exactly
        bn = torch.nn.BatchNorm2d(c, eps=2.0 ** -10).double().eval()
        with torch.no_grad():
            bn.running_var.fill_(1.0 - 2.0 ** -10)                # var + eps = 1 exactly
            bn.running_mean.zero_()
            bn.weight.copy_(scale)
            bn.bias.copy_(shift)
        s32, b32 = zoo._bn_affine(bn)
        assert s32.dtype == b32.dtype == F32 and torch.equal(s32.double(), scale) and torch.equal(b32.double(), shift)
        return bn, s32, b32

    bn1, ps, pb = bn_of(k, pick(k), torch.randint(-4, 5, (k,), generator=gen).double())
    bn2, sc, sh = bn_of(n, pick(n), torch.randn(n, generator=gen).float().double())
    ar = Arith()
    fwd = dref.d1_fwd(ar, x, ps, pb, op.w, sc, sh, act)
    nchw = lambda t: t.double().reshape(b, h, w, -1).permute(0, 3, 1, 2)
    xin = nchw(x).clone().requires_grad_(True)
    bnf = lambda t, bn: F.batch_norm(t, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
    pre = bnf(F.conv2d(torch.relu(bnf(xin, bn1)), op.w.double().reshape(n, k, 1, 1)), bn2)
    yref = torch.relu(pre) if act else pre
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(m, -1)
    assert float((dref.expected(fwd) - flat(yref.detach())).abs().max()) <= 1e-12 * (1 + float(yref.abs().max()))
    (gxref,) = torch.autograd.grad(yref, xin, nchw(g))
    y = flat(yref.detach()) if act else None
    bwd = dref.d1_bwd(ar, g, y, sc, op.wt, x, ps, pb, act)
    assert float((dref.expected(bwd) - flat(gxref)).abs().max()) <= 1e-12 * (1 + float(gxref.abs().max()))


def _emulate(row, leg, mut=()):
    """(reference Row, emulated y, emulated gx) of one row: fp32, reduction in chunks of 16, with the mutants."""
    M, K, N, act = row
    r = dref.reference_row(dref.row_name(*row), leg, M, K, N, act)
    em, o = Arith(F32, 16, mut), r.ops
    y = dref.finish(em, dref.d1_fwd(em, o.x, o.pscale, o.pshift, o.w, o.scale, o.shift, act))
    gx = dref.finish(em, dref.d1_bwd(em, o.g, r.y, o.scale, o.wt, o.x, o.pscale, o.pshift, act))
    return r, y, gx


@pytest.mark.parametrize("row", dref.ROWS, ids=str)
def test_emulation_passes_every_row_of_the_gpu_table(row):
    """The fp32 emulation (reduction in chunks of 16) passes the row's exact leg bit for bit and the gaussian bound; the
    premises (quantum, 2^23, branch shares, rounding share) are asserted on the reference alone inside `reference_row`."""
    name = dref.row_name(*row)
    exact, _ = dref.legs_of(row[3])
    r, y, gx = _emulate(row, exact)
    dref.compare_exact(name + "/fwd", y, r.fwd)
    dref.compare_exact(name + "/bwd", gx, r.bwd)
    r, y, gx = _emulate(row, "gaussian")
    rf, rb = dref.gaussian_ratio(y, r.fwd), dref.gaussian_ratio(gx, r.bwd)
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)


def test_table_covers_the_network_and_the_edges():
    assert len(dref.DENSENET_LAYERS_ALL61) == 61
    pairs = {(k, n) for k, n, _, _ in dref.DENSENET_LAYERS_ALL61}
    assert pairs == {(k, n) for _, k, n, _ in dref.NETWORK_ROWS}
    assert {(k, n, a) for k, n, _, a in dref.DENSENET_LAYERS_ALL61} == {(k, n, a) for _, k, n, a in dref.NETWORK_ROWS}
    # the two rows with ten pixel tiles and two channel tiles, forward and gradient
    order = [r for r in dref.EDGE_ROWS if r[0] > 8 * 128]
    assert order == [(1153, 24, 192, 1), (1153, 192, 24, 0)]
    for act in (0, 1):
        rows = [r for r in dref.EDGE_ROWS if r[3] == act and r not in order]
        assert {r[0] for r in rows} == {1, 127, 128, 129, 300}
        assert {r[1] for r in rows} == {8, 24, 72, 96, 992, 2048}
        assert {r[2] for r in rows} == {8, 40, 128, 136, 512}


def _rejected(row, leg, mut):
    """Does a comparator reject the mutant on this row and leg (either direction)?"""
    r, y, gx = _emulate(row, leg, (mut,))
    if leg == "gaussian":
        return dref.gaussian_ratio(y, r.fwd) > 1.0 or dref.gaussian_ratio(gx, r.bwd) > 1.0
    bad = False
    for got, want, what in ((y, r.fwd, "fwd"), (gx, r.bwd, "bwd")):
        try:
            dref.compare_exact(what, got, want)
        except AssertionError:
            bad = True
    return bad


MUTANTS = [
    # (mutant, row, leg)
    ("no_pre_relu", (127, 24, 40, 1), "clamp"), ("no_pre_relu", (127, 24, 40, 1), "gaussian"),
    ("no_pshift", (127, 24, 40, 1), "clamp"), ("no_pshift", (129, 24, 136, 0), "rounding"), ("no_pshift", (127, 24, 40, 1), "gaussian"),
    ("fma", (127, 24, 40, 1), "gaussian"), ("fma", (1, 72, 8, 0), "gaussian"), ("fma", (200, 512, 256, 0), "gaussian"),
    ("k_tail", (127, 24, 40, 1), "clamp"), ("k_tail", (129, 24, 136, 0), "rounding"), ("k_tail", (1, 8, 8, 1), "clamp"),
    ("ge_mask", (127, 24, 40, 1), "clamp"), ("ge_mask", (200, 64, 128, 1), "clamp"),
    ("no_pscale_bwd", (127, 24, 40, 1), "clamp"), ("no_pscale_bwd", (129, 24, 136, 0), "rounding"),
    ("no_pscale_bwd", (127, 24, 40, 1), "gaussian"),
    ("no_pre_mask", (127, 24, 40, 1), "clamp"), ("no_pre_mask", (129, 24, 136, 0), "rounding"),
    ("no_pre_mask", (127, 24, 40, 1), "gaussian"),
    ("row_mask", (127, 24, 40, 1), "clamp"), ("row_mask", (129, 24, 136, 0), "rounding"), ("row_mask", (127, 24, 40, 1), "gaussian"),
    ("trunc", (129, 24, 136, 0), "rounding"),
]


@pytest.mark.parametrize("mut,row,leg", MUTANTS, ids=lambda v: str(v))
def test_comparators_reject_the_mutants(mut, row, leg):
    """A kernel without the prologue ReLU, without pshift, with the prologue contracted to one fma (the header forbids it;
    the gaussian leg's contraction channels show it in the gradient's mask), without the K tail, with the output mask
    `>=`, without the pscale factor or the prologue mask in the gradient, with the prologue mask of the wrong row, or with
    truncation for RNE does not pass."""
    assert row in dref.ROWS
    assert _rejected(row, leg, mut), (mut, row, leg)
    assert not _rejected(row, leg, "none")


def test_layer_list_equals_the_network():
    """DENSENET_LAYERS_ALL61 against the (K, N, H, act) of the pre-activated 1x1 layers that zoo.DenseNet itself runs at
    224 x 224, in order."""
    from dl_attack_on_imagenet_amd import zoo
    net = zoo.DenseNet(num_classes=8).eval()
    seen = []
    for m in net.modules():
        if isinstance(m, zoo._DenseLayer):
            m.conv1.register_forward_hook(lambda mod, args, out: seen.append(
                (mod.in_channels, mod.out_channels, args[0].shape[2], 1)))
        elif isinstance(m, torch.nn.Sequential) and hasattr(m, "pool") and hasattr(m, "conv"):
            m.conv.register_forward_hook(lambda mod, args, out: seen.append(
                (mod.in_channels, mod.out_channels, args[0].shape[2], 0)))
    with torch.no_grad():
        net(torch.zeros(1, 3, 224, 224))
    assert seen == dref.DENSENET_LAYERS_ALL61


def test_rewrite_keeps_the_function_and_the_state_dict():
    """use_own_dense_pointwise_ rewrites 61 layers, leaves the state_dict keys (and values) as they are, and on CPU fp32
    the rewritten network IS the plain network, bit for bit; the tables stay fp32 under a bf16 cast."""
    from dl_attack_on_imagenet_amd import zoo
    torch.manual_seed(0)
    plain = zoo.DenseNet(num_classes=16).eval()
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in plain.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=gen))
                m.running_var.copy_(0.6 + 0.8 * torch.rand(m.num_features, generator=gen))
                m.weight.copy_(torch.randn(m.num_features, generator=gen))
    import copy
    own = copy.deepcopy(plain)
    assert zoo.use_own_dense_pointwise_(own) == 61
    assert sum(isinstance(m, zoo._OwnDenseLayer) for m in own.modules()) == 58
    assert sum(isinstance(m, zoo._OwnTransition) for m in own.modules()) == 3
    sd0, sd1 = plain.state_dict(), own.state_dict()
    assert list(sd0.keys()) == list(sd1.keys())
    assert all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    plain.load_state_dict(sd1)                                   # and it loads back
    x = torch.rand(2, 3, 64, 64, generator=gen)
    with torch.no_grad():
        assert torch.equal(plain(x), own(x))
    layer = own.features.denseblock1.denselayer1
    scale, shift = zoo._bn_affine(layer.norm1)
    assert torch.equal(layer.pscale, scale) and torch.equal(layer.pshift, shift)
    tr = own.features.transition1
    assert bool((tr.scale == 1).all()) and bool((tr.shift == 0).all()) and tr.wt2d.shape == (256, 128)
    own.to(torch.bfloat16)
    assert layer.pscale.dtype == layer.pshift.dtype == layer.scale.dtype == layer.shift.dtype == F32
    assert torch.equal(layer.pscale, scale) and layer.wt2d.dtype == torch.bfloat16
    assert torch.equal(layer.wt2d, layer.conv1.weight.reshape(128, 64).t())


def test_build_classifier_switch():
    """own_dense_pointwise is valid only for densenet121 with bf16 and channels_last; it is applied after the weights are
    loaded; own_pointwise keeps refusing DenseNet."""
    from dl_attack_on_imagenet_amd import zoo
    ok = dict(dtype=torch.bfloat16, channels_last=True, own_dense_pointwise=True, num_classes=8)
    with pytest.raises(ValueError, match="own_dense_pointwise is a switch of DenseNet-121"):
        zoo.build_classifier("mobilenet", **ok)
    with pytest.raises(ValueError, match="own_dense_pointwise is a switch of DenseNet-121"):
        zoo.build_classifier("resnet18", **ok)
    with pytest.raises(ValueError, match="own_dense_pointwise needs a bfloat16 network"):
        zoo.build_classifier("densenet121", **dict(ok, dtype=torch.float32))
    with pytest.raises(ValueError, match="own_dense_pointwise needs channels_last=True"):
        zoo.build_classifier("densenet121", **dict(ok, channels_last=False))
    with pytest.raises(ValueError):
        zoo.build_classifier("densenet121", dtype=torch.bfloat16, channels_last=True, own_pointwise=True, num_classes=8)
    model = zoo.build_classifier("densenet", **ok)
    assert sum(isinstance(m, (zoo._OwnDenseLayer, zoo._OwnTransition)) for m in model.modules()) == 61
    off = zoo.build_classifier("densenet", dtype=torch.bfloat16, channels_last=True, num_classes=8)
    assert not any(isinstance(m, (zoo._OwnDenseLayer, zoo._OwnTransition)) for m in off.modules())
    assert list(model.state_dict().keys()) == list(off.state_dict().keys())


def test_cli_switches_default_to_off():
    import demo_dL_attack
    import main
    for mod in (demo_dL_attack, main):
        p = mod.build_parser()
        assert p.parse_args([]).own_dense_pointwise == 0
        assert p.parse_args(["--own-dense-pointwise", "1"]).own_dense_pointwise == 1
