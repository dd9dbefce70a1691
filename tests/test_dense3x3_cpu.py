"""CPU: host side of the 32-channel 3x3 convolution kernels (adil_dense3x3_fwd / adil_dense3x3_bwd): the built library
exports the symbols, the header declares them and the refusals return before any device call; the fp64 restatement of
tests/classifier_reference.py against torch's convolution and autograd; the fp32 emulation of the kernel on both legs for
every row of the GPU table, with the exact leg's premises asserted on the reference alone; the comparators' power to
reject mutants; the layer list against the network itself; the `own_dense_conv` switch and the CLI default."""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dense3x3_reference as dref
from classifier_reference import F32, Arith

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"adil_dense3x3_fwd": 9, "adil_dense3x3_bwd": 9}

REFUSED_DIMS = dref.REFUSED_DIMS


def test_library_exports_and_header_declares_the_new_symbols():
    from dl_attack_on_imagenet_amd import _lib, ops
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
    assert re.search(r"#define\s+ADIL_DENSE3X3_MAX_W\s+63\b", code) and ops.DENSE3X3_MAX_W == 63
    bound = _lib.load()
    assert bound.adil_abi_version() == _lib.ABI_VERSION == 8
    # refusals need no device: they return before any HIP call
    for f in (bound.adil_dense3x3_fwd, bound.adil_dense3x3_bwd):
        for dims in REFUSED_DIMS:
            assert f(16, 16, 16, *dims, None) == -1, dims
        for i in range(3):
            null, odd = [16, 16, 16], [16, 16, 16]
            null[i], odd[i] = None, 24
            assert f(*null, 2, 4, 4, 32, 32, None) == -1, i        # each NULL pointer
            assert f(*odd, 2, 4, 4, 32, 32, None) == -1, i         # each misaligned pointer
        assert f(16, 16, 16, 2 ** 20, 2 ** 11, 1, 32, 32, None) == -1     # B H W = 2^31
        assert f(16, 16, 16, 2 ** 30, 2 ** 30, 63, 32, 32, None) == -1    # B H alone beyond 64-bit comfort


@pytest.mark.parametrize("row", [(2, 7, 7, 128, 32), (3, 6, 10, 64, 32), (2, 63, 1, 96, 32)], ids=str)
def test_restatement_equals_torch(row):
    """conv3x3 / conv3x3_bwd of tests/classifier_reference.py against F.conv2d(padding=1) and its autograd in fp64, to
    1e-12, on three rows with N = 32."""
    B, H, W, C, N = row
    op = dref.operands("restate/%s" % (row,), "gaussian", B, H, W, C, N)
    ar = Arith()
    x = op.x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(x, op.w.double(), padding=1)
    got = dref.conv3x3(ar, op.x, op.w)["y"].pre
    assert float((got - y.detach().permute(0, 2, 3, 1)).abs().max()) <= 1e-12 * (1 + float(y.detach().abs().max()))
    (gx,) = torch.autograd.grad(y, x, op.g.double().permute(0, 3, 1, 2))
    got = dref.conv3x3_bwd(ar, op.g, op.w)["gx"].pre
    assert float((got - gx.permute(0, 2, 3, 1)).abs().max()) <= 1e-12 * (1 + float(gx.abs().max()))


def _emulate(row, leg, mut=()):
    """(reference Row, emulated y, emulated gx): fp32, reduction in chunks of 16, from the packed weights, with mutants."""
    r = dref.reference_row(row, leg)
    em = Arith(F32, 16, [m for m in mut if m in ("no_wmask", "no_hmask", "trunc")])
    wp_bwd = dref.pack_bwd_unflipped(r.ops.wg) if "unflipped" in mut else r.wp_bwd
    return r, dref.emulate(em, r.ops.x, r.wp, mut), dref.emulate(em, r.ops.g, wp_bwd, mut)


@pytest.mark.parametrize("row", dref.ROWS, ids=str)
def test_emulation_passes_every_row_of_the_gpu_table(row):
    """The fp32 emulation passes the exact leg bit for bit and stays under the gaussian bound; on the reference alone: the
    exact leg's premise (inside compare_exact) and that at least 20 % of the exact outputs are no bf16 values in either
    direction, so the rounding itself is under test on every row."""
    name = dref.row_name(*row)
    r, y, gx = _emulate(row, "exact")
    for what, got, o in (("fwd", y, r.fwd), ("bwd", gx, r.bwd)):
        dref.assert_premise(name + "/" + what, o)
        assert float((o.S).max()) <= 0.03 * 2.0 ** 23
        assert dref.stats(o)[1] >= 0.20, (name, what, dref.stats(o))
        dref.compare_exact(name + "/exact/" + what, got, o)
    r, y, gx = _emulate(row, "gaussian")
    rf, rb = dref.gaussian_ratio(y, r.fwd), dref.gaussian_ratio(gx, r.bwd)
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)


def test_table_covers_the_network_and_the_tile():
    assert set(dref.DENSENET_GROWTH_LAYERS) == {(c, n, h) for _, h, _, c, n in dref.NETWORK_ROWS}
    assert {h for _, h, w, _, _ in dref.NETWORK_ROWS if h == w} == {7, 14, 28, 56}
    pixels = {b * h * w for b, h, w, _, _ in dref.ROWS}
    assert {1, 127, 128, 129, dref.TILE - 1, dref.TILE, dref.TILE + 1, 1188} <= pixels
    assert all(r in dref.ROWS for r in dref.NAN_ROWS + dref.HASH_ROWS + [dref.MASK_ROW])


def _rejected(row, mut):
    r, y, gx = _emulate(row, "exact", (mut,))
    bad = False
    for got, want, what in ((y, r.fwd, "fwd"), (gx, r.bwd, "bwd")):
        try:
            dref.compare_exact(what, got, want)
        except AssertionError:
            bad = True
    return bad


@pytest.mark.parametrize("mut", ["no_wmask", "no_hmask", "trunc", "unflipped", "tap_transposed"])
@pytest.mark.parametrize("row", [(3, 6, 10, 64, 32), (1, 3, 63, 32, 64)], ids=str)
def test_comparators_reject_the_mutants(mut, row):
    """A kernel without the left / top mask, with truncation for RNE, with unflipped taps in the gradient pack or with the
    tap index kw * 3 + kh does not pass the exact leg; the unmutated emulation does."""
    assert row in dref.ROWS
    assert _rejected(row, mut), (mut, row)
    assert not _rejected(row, "none")


def test_layer_list_equals_the_network():
    """DENSENET_GROWTH_LAYERS against the (C, N, H) of the 3x3 convolutions that zoo.DenseNet itself runs at 224 x 224."""
    from dl_attack_on_imagenet_amd import zoo
    net = zoo.DenseNet(num_classes=8).eval()
    seen = []
    for m in net.modules():
        if isinstance(m, zoo._DenseLayer):
            m.conv2.register_forward_hook(lambda mod, args, out: seen.append(
                (mod.in_channels, mod.out_channels, args[0].shape[2])))
    with torch.no_grad():
        net(torch.zeros(1, 3, 224, 224))
    assert len(seen) == 58 and seen == dref.DENSENET_GROWTH_LAYERS


@pytest.mark.parametrize("pointwise", ["plain", "pointwise_first", "pointwise_after"])
def test_rewrite_keeps_the_function_and_the_state_dict(pointwise):
    """use_own_dense_conv_ rewrites 58 modules on a plain network and on an own_dense_pointwise network (either order),
    leaves the state_dict keys and values as they are, and on CPU fp32 the rewritten network IS the plain network, bit for
    bit; the packed buffers are bf16, 2-D and follow the weight."""
    from dl_attack_on_imagenet_amd import ops, zoo
    torch.manual_seed(0)
    plain = zoo.DenseNet(num_classes=16).eval()
    own = copy.deepcopy(plain)
    if pointwise == "pointwise_first":
        assert zoo.use_own_dense_pointwise_(own) == 61
    assert zoo.use_own_dense_conv_(own) == 58
    assert zoo.use_own_dense_conv_(own) == 0                       # nothing left to rewrite
    if pointwise == "pointwise_after":
        assert zoo.use_own_dense_pointwise_(own) == 61
    assert sum(isinstance(m, zoo._OwnGrowthConv) for m in own.modules()) == 58
    assert sum(isinstance(m, zoo._OwnDenseLayer) for m in own.modules()) == (0 if pointwise == "plain" else 58)
    sd0, sd1 = plain.state_dict(), own.state_dict()
    assert list(sd0.keys()) == list(sd1.keys())
    assert all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    plain.load_state_dict(sd1)                                   # and it loads back
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        assert torch.equal(plain(x), own(x))
    conv = own.features.denseblock1.denselayer1.conv2
    wp_fwd, wp_bwd = ops.pack_conv3x3_weights(conv.weight)
    assert conv.wp_fwd.shape == (32, 9 * 128) and conv.wp_bwd.shape == (128, 9 * 32)
    assert conv.wp_fwd.dtype == conv.wp_bwd.dtype == torch.bfloat16
    assert torch.equal(conv.wp_fwd, wp_fwd) and torch.equal(conv.wp_bwd, wp_bwd)
    assert torch.equal(wp_fwd.reshape(32, 9, 128), dref.pack_taps(conv.weight.detach().bfloat16()))
    assert torch.equal(wp_bwd.reshape(128, 9, 32), dref.pack_taps_flipped(conv.weight.detach().bfloat16()))
    own.to(torch.bfloat16)
    assert conv.weight.dtype == torch.bfloat16 and torch.equal(conv.wp_fwd, wp_fwd)
    with torch.no_grad():                                        # a bf16 CPU input takes F.conv2d on the weight as well
        xin = torch.randn(1, 128, 5, 5).bfloat16()
        assert torch.equal(conv(xin), F.conv2d(xin, conv.weight, padding=1))


def test_build_classifier_switch():
    """own_dense_conv is valid only for densenet121 with bf16 and channels_last; it is independent of own_dense_pointwise."""
    from dl_attack_on_imagenet_amd import zoo
    ok = dict(dtype=torch.bfloat16, channels_last=True, own_dense_conv=True, num_classes=8)
    with pytest.raises(ValueError, match="own_dense_conv is a switch of DenseNet-121"):
        zoo.build_classifier("mobilenet", **ok)
    with pytest.raises(ValueError, match="own_dense_conv needs a bfloat16 network"):
        zoo.build_classifier("densenet121", **dict(ok, dtype=torch.float32))
    with pytest.raises(ValueError, match="own_dense_conv needs channels_last=True"):
        zoo.build_classifier("densenet121", **dict(ok, channels_last=False))
    off = zoo.build_classifier("densenet", dtype=torch.bfloat16, channels_last=True, num_classes=8)
    assert not any(isinstance(m, zoo._OwnGrowthConv) for m in off.modules())
    for both in (False, True):
        model = zoo.build_classifier("densenet", own_dense_pointwise=both, **ok)
        assert sum(isinstance(m, zoo._OwnGrowthConv) for m in model.modules()) == 58
        assert sum(isinstance(m, zoo._OwnDenseLayer) for m in model.modules()) == (58 if both else 0)
        assert list(model.state_dict().keys()) == list(off.state_dict().keys())
        assert all(m.wp_fwd.dtype == torch.bfloat16 for m in model.modules() if isinstance(m, zoo._OwnGrowthConv))


def test_cli_switches_default_to_off():
    import demo_dL_attack
    import main
    for mod in (demo_dL_attack, main):
        p = mod.build_parser()
        assert p.parse_args([]).own_dense_conv == 0
        assert p.parse_args(["--own-dense-conv", "1"]).own_dense_conv == 1
