"""CPU: host side of the VGG kernels (adil_conv3x3_wide, adil_bias_relu_pool2_fwd / _bwd): the built library exports the
symbols, the header declares them and the refusals return before any device call; the fp32 emulation of the 2-D tiling on
both legs for every row of the GPU table, with the exact leg's premises asserted on the reference alone; the comparators'
power to reject mutants; the pool restatement against torch's own fp32 chain and autograd, bit for bit, with its premises
and mutants; the `own_vgg_conv` switch, the CLI flag and the switched network on the CPU."""
import ctypes
import os
import re

import pytest
import torch

import vgg_conv_reference as vref
from classifier_reference import F32, Arith

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"adil_conv3x3_wide": 9, "adil_bias_relu_pool2_fwd": 9, "adil_bias_relu_pool2_bwd": 8}


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
    assert _lib.load().adil_abi_version() == _lib.ABI_VERSION == 8


def test_wide_conv_refusals_need_no_device():
    """Every refusal returns ADIL_EINVAL before any HIP call: C or N of 32, 96 or 0; W, H or B of 0 or -1; 2^31 pixels; a
    weight pack of 2^31 elements; each pointer null or misaligned."""
    from dl_attack_on_imagenet_amd import _lib
    f = _lib.load().adil_conv3x3_wide
    for dims in vref.REFUSED_DIMS:
        assert f(16, 16, 16, *dims, None) == -1, dims
    for i in range(3):
        null, odd = [16, 16, 16], [16, 16, 16]
        null[i], odd[i] = None, 24
        assert f(*null, 2, 4, 4, 64, 64, None) == -1, i
        assert f(*odd, 2, 4, 4, 64, 64, None) == -1, i
    assert f(16, 16, 16, 2 ** 20, 2 ** 11, 1, 64, 64, None) == -1          # B H W = 2^31
    assert f(16, 16, 16, 2 ** 30, 2 ** 30, 70, 64, 64, None) == -1         # B H alone beyond 32 bits
    assert f(16, 16, 16, 1, 4, 4, 2 ** 14, 2 ** 14, None) == -1            # 9 C N >= 2^31


def test_pool_refusals_need_no_device():
    """Odd H, odd W, C = 12, a zero or negative size, 2^31 pixels, each pointer null or misaligned; a NULL bias alone is
    accepted as far as the check goes (that call is not made here: it would launch)."""
    from dl_attack_on_imagenet_amd import _lib
    lib = _lib.load()
    fwd, bwd = lib.adil_bias_relu_pool2_fwd, lib.adil_bias_relu_pool2_bwd
    for dims in vref.POOL_REFUSED_DIMS:
        assert fwd(16, 16, 16, 16, *dims, None) == -1, dims
        assert fwd(16, None, 16, 16, *dims, None) == -1, dims
        assert bwd(16, 16, 16, *dims, None) == -1, dims
    for i, odd in ((0, 24), (1, 24), (2, 24), (3, 20)):
        a = [16, 16, 16, 16]
        a[i] = odd
        assert fwd(*a, 2, 4, 4, 8, None) == -1, i
        if i != 1:
            a[i] = None
            assert fwd(*a, 2, 4, 4, 8, None) == -1, i
    for i, odd in ((0, 24), (1, 20), (2, 24)):
        null, bad = [16, 16, 16], [16, 16, 16]
        null[i], bad[i] = None, odd
        assert bwd(*null, 2, 4, 4, 8, None) == -1, i
        assert bwd(*bad, 2, 4, 4, 8, None) == -1, i
    assert fwd(16, 16, 16, 16, 2 ** 20, 2 ** 10, 2, 8, None) == -1          # B H W = 2^31
    assert bwd(16, 16, 16, 2 ** 20, 2 ** 10, 2, 8, None) == -1


def _emulate(row, leg, mut=()):
    """(reference Row, emulated y, emulated gx): fp32, reduction in chunks of 16, from the packed weights, with mutants."""
    r = vref.reference_row(row, leg)
    em = Arith(F32, 16, [m for m in mut if m == "trunc"])
    wp_bwd = vref.pack_bwd_unflipped(r.ops.wg) if "unflipped" in mut else r.wp_bwd
    return r, vref.emulate(em, r.ops.x, r.wp, mut), vref.emulate(em, r.ops.g, wp_bwd, mut)


@pytest.mark.parametrize("row", vref.ROWS, ids=str)
def test_emulation_passes_every_row_of_the_gpu_table(row):
    """The fp32 emulation of the 2-D tiling with a zero-filled halo passes the exact leg bit for bit and stays under the
    gaussian bound; on the reference alone: the exact leg's premise and that at least 20 % of the exact outputs are no
    bf16 values in either direction, so the rounding itself is under test on every row."""
    name = vref.row_name(*row)
    r, y, gx = _emulate(row, "exact")
    for what, got, o in (("fwd", y, r.fwd), ("bwd", gx, r.bwd)):
        vref.assert_premise(name + "/" + what, o)
        assert float((o.S).max()) < 2.0 ** 20
        assert vref.stats(o)[1] >= 0.20, (name, what, vref.stats(o))
        vref.compare_exact(name + "/exact/" + what, got, o)
    r, y, gx = _emulate(row, "gaussian")
    rf, rb = vref.gaussian_ratio(y, r.fwd), vref.gaussian_ratio(gx, r.bwd)
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)


def test_table_covers_the_issue_the_network_and_the_tiles():
    rows = set(vref.ROWS)
    assert set(vref.ISSUE_ROWS) <= rows and len(vref.ISSUE_ROWS) == 10
    assert all(r in rows for r in vref.NAN_ROWS + vref.HASH_ROWS)
    for th in (8, 16):                                    # TH - 1, TH, TH + 1 rows and TW - 1, TW, TW + 1 columns, per tile shape
        shape = {(h, w) for _, h, w, c, n in vref.ROWS for o in (c, n) if vref.tile_rows(o) == th}
        assert {(th - 1, vref.TW - 1), (th, vref.TW), (th + 1, vref.TW + 1)} <= shape, th
    assert (64, 128, 112) in {(c, n, w) for _, _, w, c, n in vref.ROWS}          # layer 2 of the network


def _rejected(row, mut):
    r, y, gx = _emulate(row, "exact", (mut,))
    bad = False
    for got, want, what in ((y, r.fwd, "fwd"), (gx, r.bwd, "bwd")):
        try:
            vref.compare_exact(what, got, want)
        except AssertionError:
            bad = True
    return bad


@pytest.mark.parametrize("mut", ["no_right_fill", "no_bottom_fill", "origin_off_by_one", "unflipped", "tap_transposed", "trunc"])
@pytest.mark.parametrize("row", vref.NAN_ROWS, ids=str)
def test_comparators_reject_the_mutants(mut, row):
    """A kernel without the zero fill at the right or at the bottom edge, with the halo origin off by one, with unflipped
    taps in the gradient pack, with the tap index kw * 3 + kh or with truncation for RNE does not pass the exact leg; the
    unmutated emulation does."""
    assert row in vref.ROWS
    assert _rejected(row, mut), (mut, row)
    assert not _rejected(row, "none")


# ------------------------------------------------------------------------------------------------------------ pool pair
POOL_CASES = [(row, bias) for row in vref.POOL_ROWS for bias in (True, False)]


@pytest.mark.parametrize("row,bias", POOL_CASES, ids=str)
@pytest.mark.parametrize("leg", ["tie", "gaussian"])
def test_pool_restatement_equals_torch_bitwise(row, bias, leg):
    """The straight-line rule (first strictly greater wins, index 4 for a dead window) equals torch's fp32 chain
    max_pool2d(relu(x.float() + bias), 2) rounded to bf16 and its autograd, bit for bit, zeros' signs included."""
    r = vref.pool_reference(row, bias, leg)
    got = vref.pool_restate(r.ops)
    assert vref.same_bits(got.y, r.y)
    assert vref.same_bits(got.gx, r.gx)
    assert int(got.idx.max()) <= 4 and bool(((got.idx == 4) == (got.y == 0)).all())


def test_pool_premises_on_the_reference_alone():
    """Tie leg: at least 10 % live windows with tied maxima and at least 5 % dead windows on every row of 100 windows or
    more (the 1 x 2 x 2 x 8 row has eight) and over the whole table; every index value 0-4 occurs on each of those rows."""
    tied = dead = total = 0.0
    for row, bias in POOL_CASES:
        r = vref.pool_reference(row, bias, "tie")
        n = r.y.numel()
        tied, dead, total = tied + r.live_tied * n, dead + r.dead * n, total + n
        if n >= 100:
            assert r.live_tied >= 0.10 and r.dead >= 0.05, (row, bias, r.live_tied, r.dead)
            assert set(vref.pool_restate(r.ops).idx.unique().tolist()) == {0, 1, 2, 3, 4}, (row, bias)
    assert tied / total >= 0.10 and dead / total >= 0.05


@pytest.mark.parametrize("mut", ["last_winner", "dead_passes", "bias_after_max"])
def test_pool_mutants_are_rejected(mut):
    """Last winner instead of first, a dead window that passes its gradient, the bias added after the maximum: each
    differs from torch on the tie leg of the (2, 6, 10, 16) row with bias; the unmutated rule does not."""
    r = vref.pool_reference((2, 6, 10, 16), True, "tie")
    got = vref.pool_restate(r.ops, (mut,))
    assert not (vref.same_bits(got.y, r.y) and vref.same_bits(got.gx, r.gx)), mut
    ok = vref.pool_restate(r.ops)
    assert vref.same_bits(ok.y, r.y) and vref.same_bits(ok.gx, r.gx)


# ------------------------------------------------------------------------------------------------ switch, CLI, network
def test_build_classifier_switch():
    """own_vgg_conv is valid only for vgg11 with bf16 and channels_last."""
    from dl_attack_on_imagenet_amd import zoo
    ok = dict(dtype=torch.bfloat16, channels_last=True, own_vgg_conv=True, num_classes=8)
    with pytest.raises(ValueError, match="own_vgg_conv is a switch of VGG11"):
        zoo.build_classifier("resnet18", **ok)
    with pytest.raises(ValueError, match="own_vgg_conv needs a bfloat16 network"):
        zoo.build_classifier("vgg11", **dict(ok, dtype=torch.float32))
    with pytest.raises(ValueError, match="own_vgg_conv needs channels_last=True"):
        zoo.build_classifier("vgg11", **dict(ok, channels_last=False))
    with pytest.raises(ValueError):
        zoo.use_own_vgg_conv_(zoo.build_classifier("mobilenet", num_classes=8)[1])
    (row,) = zoo.VGG_SWITCHES
    assert row.keyword == "own_vgg_conv" and row.flag == "--own-vgg-conv" and row.network == "vgg11"
    assert row.bf16 and row.channels_last and zoo.NETWORK_LABELS["vgg11"] == "VGG11"
    assert row.keyword in zoo.build_classifier.__doc__ and row.help in zoo.build_classifier.__doc__
    assert "own_vgg_conv" not in [r.keyword for r in zoo.SWITCHES]


def _demo(argv):
    import demo_dL_attack
    args = demo_dL_attack.build_parser().parse_args(argv)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    return demo_dL_attack.classifier_keywords(args, args.model.lower(), dtype)


def test_cli_flag_and_keywords():
    """--own-vgg-conv defaults to 0 and refuses 2; on vgg in bf16 it gives own_vgg_conv=True and channels_last=True; every
    other network keeps exactly the dictionary it had (the keys of zoo.SWITCHES and the four of the fast path)."""
    import demo_dL_attack
    from dl_attack_on_imagenet_amd import zoo
    p = demo_dL_attack.build_parser()
    assert p.parse_args([]).own_vgg_conv == 0 and p.parse_args(["--own-vgg-conv", "1"]).own_vgg_conv == 1
    with pytest.raises(SystemExit):
        p.parse_args(["--own-vgg-conv", "2"])
    off = {r.keyword: False for r in zoo.SWITCHES}
    not_fast = dict(fuse_bn_act=False, fuse_stem=False, own_strided_conv=False)
    assert _demo(["-m", "vgg", "--dtype", "bf16", "--own-vgg-conv", "1"]) == dict(
        off, own_vgg_conv=True, channels_last=True, **not_fast)
    assert _demo(["-m", "vgg", "--dtype", "bf16"]) == dict(off, own_vgg_conv=False, channels_last=False, **not_fast)
    assert _demo(["-m", "vgg", "--dtype", "fp32", "--own-vgg-conv", "1"]) == dict(
        off, own_vgg_conv=False, channels_last=False, **not_fast)
    for model in ("densenet", "mobilenet", "vit"):
        assert _demo(["-m", model, "--dtype", "bf16", "--own-vgg-conv", "1"]) == dict(off, channels_last=False, **not_fast)
    assert _demo(["-m", "resnet50", "--dtype", "bf16", "--own-vgg-conv", "1"]) == dict(
        off, head_fp32="inference", channels_last=True, fuse_bn_act=True, fuse_stem=True, own_strided_conv=False)


def test_switched_network_on_the_cpu():
    """A switched bf16 VGG11 built on the CPU has the plain network's state-dict keys, loads its state dict, holds the same
    children under the same names, keeps its bias tables fp32 and its packs bf16 (non-persistent), and gives the plain
    network's output bit for bit on a CPU input, where every group falls back; with the padded first convolution too."""
    from dl_attack_on_imagenet_amd import ops, zoo
    kw = dict(num_classes=8, dtype=torch.bfloat16, channels_last=True)
    plain = zoo.build_classifier("vgg11", **kw)
    own = zoo.build_classifier("vgg11", own_vgg_conv=True, **kw)
    feats = own[1].features
    assert isinstance(feats, zoo._OwnVggFeatures) and isinstance(feats, torch.nn.Sequential)
    assert [(n, type(m)) for n, m in feats.named_children()] == [(n, type(m)) for n, m in plain[1].features.named_children()]
    assert [(c, n, p) for c, n, _, p in vref.VGG11_GROUPS] == [
        (feats._modules[g[0]].in_channels, feats._modules[g[0]].out_channels, g[2] is not None) for g in feats._groups]
    sd0, sd1 = plain.state_dict(), own.state_dict()
    assert list(sd0) == list(sd1) and all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    own.load_state_dict(sd0)
    packed = [g[0] for g in feats._groups][1:]
    assert sorted(feats._buffers) == sorted(f"{k}_{n}" for n in packed for k in ("wp_fwd", "wp_bwd", "bias", "ones"))
    for n in packed:
        conv = feats._modules[n]
        wf, wb = ops.pack_conv3x3_weights(conv.weight)
        assert torch.equal(feats._buffers[f"wp_fwd_{n}"], wf) and torch.equal(feats._buffers[f"wp_bwd_{n}"], wb)
        assert wf.dtype == torch.bfloat16 and feats._buffers[f"bias_{n}"].dtype == torch.float32
        assert torch.equal(feats._buffers[f"bias_{n}"].bfloat16(), conv.bias)       # the fp32 value the bf16 bias came from
        assert torch.equal(feats._buffers[f"ones_{n}"], torch.ones(conv.out_channels))
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).bfloat16().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        want = plain(x)
        assert torch.equal(own(x), want)
        padded = zoo.build_classifier("vgg11", own_vgg_conv=True, pad_input_channels=8, **kw)
        assert isinstance(padded[1].features[0], zoo.ChannelPaddedConv)
        assert torch.equal(padded(x), zoo.build_classifier("vgg11", pad_input_channels=8, **kw)(x))
