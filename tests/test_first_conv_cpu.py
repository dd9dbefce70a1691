"""CPU: host side of the first-convolution kernels (adil_first3x3_fwd / adil_first3x3_bwd): the built library exports the
symbols and the header declares them, the fp64 restatement of tests/first_conv_reference.py against torch's convolution,
BatchNorm, hardtanh and autograd, the fp32 emulation of the kernel's own order on every leg for every row of the GPU table,
the vacuity assertions of the exact legs on the reference alone, the exact legs' power to reject mutants, the weight
packing, the `own_first_conv` switch and the CLI default."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import first_conv_reference as fref
from classifier_reference import BF16, F32, F64, Arith

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"adil_first3x3_fwd": 17, "adil_first3x3_bwd": 14}


def test_library_exports_and_header_declares_the_new_symbols():
    from dl_attack_on_imagenet_amd import _lib
    from dl_attack_on_imagenet_amd.build import build_library
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIBPATH)
    src = open(os.path.join(ROOT, "include", "adil_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        assert not name.startswith("adil_conv3x3")                     # the recorded-call table claims that prefix
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    bound = _lib.load()
    assert bound.adil_abi_version() == _lib.ABI_VERSION == 8
    # refusals need no device: they return before any HIP call
    f, b = bound.adil_first3x3_fwd, bound.adil_first3x3_bwd
    nm = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    fwd = lambda x, dt, w, sc, sh, y, B, H, W, r: f(x, dt, w, *nm, sc, sh, y, B, H, W, r, None)
    bwd = lambda g, y, sc, w, gx, dt, B, H, W, r: b(g, y, sc, w, *nm[3:], gx, dt, B, H, W, r, None)
    assert fwd(None, 0, None, None, None, None, 1, 8, 8, 1) == -1
    assert bwd(None, None, None, None, None, 0, 1, 8, 8, 1) == -1
    for (B, H, W, dt, r) in [(0, 8, 8, 0, 1), (-1, 8, 8, 1, 1), (1, 0, 8, 0, 1), (1, 8, 0, 1, 0), (1, 8, 8, 2, 1), (1, 8, 8, -1, 1),
                             (1, 8, 8, 0, 2), (1, 8, 8, 1, -1)]:
        assert fwd(16, dt, 16, 16, 16, 16, B, H, W, r) == -1, (B, H, W, dt, r)
        assert bwd(16, 16, 16, 16, 16, dt, B, H, W, r) == -1, (B, H, W, dt, r)
    for i in range(5):                                                 # each NULL mandatory pointer in turn
        a = [16] * 5
        a[i] = None
        assert fwd(a[0], 0, a[1], a[2], a[3], a[4], 1, 8, 8, 1) == -1
        assert bwd(a[0], a[1], a[2], a[3], a[4], 0, 1, 8, 8, 1) == -1
    assert fwd(16, 0, 16, 16, 16, 24, 1, 8, 8, 1) == -1                # misaligned y
    assert fwd(16, 0, 24, 16, 16, 16, 1, 8, 8, 1) == -1                # misaligned w_fwd
    assert fwd(18, 0, 16, 16, 16, 16, 1, 8, 8, 1) == -1                # fp32 x on a 2-byte boundary
    assert fwd(17, 1, 16, 16, 16, 16, 1, 8, 8, 1) == -1                # bf16 x on an odd address
    assert bwd(24, 16, 16, 16, 16, 0, 1, 8, 8, 1) == -1                # misaligned g
    assert bwd(16, 24, 16, 16, 16, 0, 1, 8, 8, 1) == -1                # misaligned y
    assert bwd(16, 16, 16, 24, 16, 0, 1, 8, 8, 1) == -1                # misaligned w_bwd
    assert bwd(16, 16, 16, 16, 18, 0, 1, 8, 8, 1) == -1                # fp32 gx on a 2-byte boundary
    assert bwd(16, 16, 16, 16, 17, 1, 1, 8, 8, 1) == -1                # bf16 gx on an odd address


CASES = [(2, 5, 7, 1), (1, 1, 1, 1), (3, 4, 4, 0), (1, 9, 6, 1), (2, 8, 8, 1), (1, 33, 17, 0)]


@pytest.mark.parametrize("b,h,w,relu6", CASES)
def test_restatement_equals_torch(b, h, w, relu6):
    """fp64: first_fwd against F.conv2d on the normalised input + F.batch_norm (eval) + hardtanh(0, 6), first_bwd against
    autograd.  x is given as bf16 values whose normalisation by a power-of-two inv_std and an integer-grid mean is exact, and
    the scales are +-1/2, +-1, +-2, so that the kernel's two roundings (x', gz) are the identity and torch computes the same
    function; to 1e-12."""
    name = "restate/%s" % ((b, h, w, relu6),)
    ex = fref.operands(name, "clamp", b, h, w, BF16)
    ga = fref.operands(name, "gaussian", b, h, w, BF16)
    wgt = ga.w
    gen = torch.Generator().manual_seed(3)
    bn = torch.nn.BatchNorm2d(32).double().eval()
    with torch.no_grad():
        bn.bias.copy_(torch.randn(32, generator=gen))
        bn.running_mean.copy_(torch.randn(32, generator=gen))
        bn.running_var.copy_(torch.rand(32, generator=gen) + 0.1)
        bn.weight.copy_(ex.scale.double() * torch.sqrt(bn.running_var + bn.eps))
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    shift = bn.bias.detach() - bn.running_mean * scale
    assert float((scale - ex.scale.double()).abs().max()) < 1e-14
    mean = torch.tensor(ex.mean, dtype=F64).view(1, 3, 1, 1)
    istd = torch.tensor(ex.inv_std, dtype=F64).view(1, 3, 1, 1)
    xin = ex.x.double().clone().requires_grad_(True)
    pre = F.batch_norm(F.conv2d((xin - mean) * istd, wgt.double(), None, 2, 1), bn.running_mean, bn.running_var, bn.weight,
                       bn.bias, False, 0.0, bn.eps)
    yref = F.hardtanh(pre, 0.0, 6.0) if relu6 else pre
    ar = Arith()
    o = fref.first_fwd(ar, ex.x, wgt, ex.mean, ex.inv_std, ex.scale, shift, relu6)
    yr = yref.detach().permute(0, 2, 3, 1)
    assert o.n == 27 and o.pre.shape == yr.shape == (b,) + fref.out_grid(h, w) + (32,)
    assert float((fref.expected(o) - yr).abs().max()) <= 1e-12 * max(1.0, float(yr.abs().max()))
    g = ex.g.double().permute(0, 3, 1, 2)
    (gref,) = torch.autograd.grad(yref, xin, g)
    for dt in (BF16, F32):
        ob = fref.first_bwd(ar, ex.g, yr if relu6 else None, ex.scale, wgt, ex.inv_std, h, w, relu6, dt)
        assert ob.n == 128 and ob.pre.shape == gref.shape and ob.dtype == dt
        assert float((ob.pre - gref).abs().max()) <= 1e-10 * max(1.0, float(gref.abs().max()))


def _emu_fwd(emu, op, relu6):
    return fref.finish(emu, fref.first_fwd(emu, op.x, op.w, op.mean, op.inv_std, op.scale, op.shift, relu6))


def _emu_bwd(emu, op, y, H, W, relu6, dtype):
    return fref.finish(emu, fref.first_bwd(emu, op.g, y, op.scale, op.w, op.inv_std, H, W, relu6, dtype))


ALL_ROWS = fref.ROWS + [(b, h, w, dt, 1) for b, h, w in fref.NAN_ROWS for dt in (BF16,)]


@pytest.mark.parametrize("row", ALL_ROWS, ids=str)
def test_emulation_passes_every_leg_and_the_premises_hold(row):
    """Every row of the GPU table, with the kernel replaced by its fp32 emulation (one partial sum per tap row, the
    kernel's own order): the vacuity assertions (premise, 5 % per ReLU6 branch in the pre-activation and in the gradient's
    mask, 10 % of the rounding set's x' and y inexact) on the reference alone, then bit for bit on the exact legs and under
    the bound on the gaussian leg."""
    B, H, W, dtype, relu6 = row
    emu = Arith(F32, chunk=16)
    for leg in fref.exact_legs(relu6):
        name = fref.row_name(row, leg)
        a = 1 if leg == "clamp" else 0
        op, y, ref, refb = fref.exact_references(name, leg, B, H, W, dtype)
        fref.compare_exact(name + "/fwd", _emu_fwd(emu, op, a), ref)
        fref.compare_exact(name + "/bwd", _emu_bwd(emu, op, y, H, W, a, dtype), refb)
    name = fref.row_name(row, "gaussian")
    op = fref.operands(name, "gaussian", B, H, W, dtype)
    ref = fref.first_fwd(Arith(), op.x, op.w, op.mean, op.inv_std, op.scale, op.shift, relu6)
    got = _emu_fwd(emu, op, relu6)
    rf = fref.gaussian_ratio(got, ref)
    y = got.to(BF16) if relu6 else None
    refb = fref.first_bwd(Arith(), op.g, y, op.scale, op.w, op.inv_std, H, W, relu6, dtype)
    rb = fref.gaussian_ratio(_emu_bwd(emu, op, y, H, W, relu6, dtype), refb)
    print(name, "max |err| / bound: fwd %.3f bwd %.3f" % (rf, rb))
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)


def test_row_sets_hold_what_they_claim():
    rows = fref.ROWS
    shapes = {(r[1], r[2]) for r in rows}
    assert {(1, 1), (2, 3), (7, 9), (8, 8), (33, 17)} <= shapes and (1, 1, 1) in {r[:3] for r in rows}
    th, tw = fref.FWD_TILE
    assert {th - 1, th, th + 1} <= {fref.out_grid(r[1], r[2])[0] for r in rows}
    assert {tw - 1, tw, tw + 1} <= {fref.out_grid(r[1], r[2])[1] for r in rows}
    th, tw = fref.BWD_TILE
    assert {th - 1, th, th + 1} <= {r[1] for r in rows} and {tw - 1, tw, tw + 1} <= {r[2] for r in rows}
    assert {r[3] for r in rows} == {BF16, F32} and {r[4] for r in rows} == {0, 1}
    assert sum(r[:3] == (1, 224, 224) for r in rows) == 1
    assert any(r[0] > 1 and (fref.out_grid(r[1], r[2])[0] > fref.FWD_TILE[0] - 1 or r[2] >= fref.BWD_TILE[1]) for r in rows)
    assert len(fref.NAN_ROWS) == 2 and fref.NAN_ROWS[0][1] % 2 == 1 and fref.NAN_ROWS[0][2] % 2 == 1
    b, h, w = fref.NAN_ROWS[1]
    assert fref.out_grid(h, w)[0] > fref.FWD_TILE[0] and fref.out_grid(h, w)[1] > fref.FWD_TILE[1]
    assert h > fref.BWD_TILE[0] and w > fref.BWD_TILE[1]


MUTANT_ROWS = [(3, 7, 9, BF16, 1), (2, 8, 8, F32, 1), (1, 17, 33, BF16, 0), (1, 17, 33, F32, 1)]
MUTANTS = ["raw_pad", "no_round_x", "trunc", "mean_sign", "chan_order", "neg_zero", "flip_taps", "parity", "no_inv_std",
           "no_scale_bwd", "ge_mask", "le_mask"]


def _exact_leg(emu):
    """The exact legs of tests/test_gpu_first_conv.py with the kernel replaced by the emulation `emu`; returns the names of
    the comparisons that failed."""
    failed = []
    for row in MUTANT_ROWS:
        B, H, W, dtype, relu6 = row
        for leg in fref.exact_legs(relu6):
            name = fref.row_name(row, leg)
            a = 1 if leg == "clamp" else 0
            op, y, ref, refb = fref.exact_references(name, leg, B, H, W, dtype)
            for what, o, got in (("fwd", ref, lambda: _emu_fwd(emu, op, a)),
                                 ("bwd", refb, lambda: _emu_bwd(emu, op, y, H, W, a, dtype))):
                try:
                    fref.compare_exact(name + "/" + what, got(), o)
                except AssertionError:
                    failed.append(name + "/" + what)
    return failed


def test_exact_leg_passes_the_emulation_and_rejects_mutants():
    assert _exact_leg(Arith(F32, chunk=16)) == []
    assert len(MUTANTS) >= 10
    for m in MUTANTS:
        failed = _exact_leg(Arith(F32, chunk=16, mut=(m,)))
        print(m, "rejected by", len(failed), "comparisons, e.g.", failed[:2])
        assert failed, "mutant %s passes the exact leg" % m


def test_pack_first3x3_weights_round_trips_and_refuses_other_shapes():
    from dl_attack_on_imagenet_amd import ops
    w = torch.randn(32, 3, 3, 3, generator=torch.Generator().manual_seed(2))
    wf, wb = ops.pack_first3x3_weights(w)
    assert wf.shape == (32, 48) and wb.shape == (3, 288) and wf.dtype == wb.dtype == BF16
    assert wf.is_contiguous() and wb.is_contiguous()
    wf4, wb3 = wf.reshape(32, 3, 4, 4), wb.reshape(3, 9, 32)
    assert torch.equal(wf4[:, :, :3, :3].permute(0, 3, 1, 2), w.bfloat16())          # [n][kh][kw][c] -> [n][c][kh][kw]
    assert bool((wf4[:, :, 3] == 0).all()) and bool((wf4[:, :, :, 3] == 0).all())
    assert torch.equal(wb3.reshape(3, 3, 3, 32).permute(3, 0, 1, 2), w.bfloat16())   # [c][kh][kw][n] -> [n][c][kh][kw]
    assert torch.equal(wf4, fref.pack_fwd(w.bfloat16())) and torch.equal(wb3, fref.pack_bwd(w.bfloat16()))
    for shape in [(64, 3, 3, 3), (32, 4, 3, 3), (32, 3, 7, 7), (32, 3, 3), (32, 27)]:
        with pytest.raises(ValueError):
            ops.pack_first3x3_weights(torch.zeros(shape))
    x = torch.zeros(2, 3, 8, 8)
    assert not ops.first_conv3x3_covers(x)                                           # not on a GPU
    with pytest.raises(ValueError):
        ops.first_conv3x3(x, wf, wb, torch.zeros(32), torch.zeros(32), (0, 0, 0), (1, 1, 1))


def _net(model):
    return model[-1]


def test_switch_rewrites_the_first_layer_and_nothing_else(tmp_path):
    from dl_attack_on_imagenet_amd import zoo
    kw = dict(num_classes=10, seed=1, dtype=torch.bfloat16, channels_last=True)
    with pytest.raises(ValueError, match="own_first_conv"):
        zoo.build_classifier("resnet18", own_first_conv=True, **kw)
    with pytest.raises(ValueError, match="own_first_conv"):
        zoo.build_classifier("mobilenet", num_classes=10, seed=1, channels_last=True, own_first_conv=True)
    with pytest.raises(ValueError, match="own_first_conv"):
        zoo.build_classifier("mobilenet", num_classes=10, seed=1, dtype=torch.bfloat16, own_first_conv=True)
    with pytest.raises(ValueError):
        zoo.use_own_first_conv_(zoo.build_classifier("resnet18", num_classes=10, seed=1)[1], (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        zoo._OwnFirstConv(zoo._ConvBNReLU6(3, 32, 3, 1), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        zoo._OwnFirstConv(zoo._ConvBNReLU6(32, 32, 3, 2, 32), (0, 0, 0), (1, 1, 1))
    plain = zoo.build_classifier("mobilenet", num_classes=10, seed=1)
    off = zoo.build_classifier("mobilenet", **kw)
    off2 = zoo.build_classifier("mobilenet", own_first_conv=False, **kw)
    on = zoo.build_classifier("mobilenet", own_first_conv=True, **kw)
    all3 = zoo.build_classifier("mobilenet", own_first_conv=True, own_depthwise=True, own_pointwise=True, **kw)
    assert [type(m) for m in off.modules()] == [type(m) for m in off2.modules()] == [type(m) for m in plain.modules()]
    assert isinstance(off[0], zoo.Normalize) and len(off) == 2
    for net in (on, all3):
        assert len(net) == 1 and isinstance(net[0], zoo.MobileNetV2)                  # the module normalises
        first = net[0].features[0]
        assert isinstance(first, zoo._OwnFirstConv) and sum(isinstance(m, zoo._OwnFirstConv) for m in net.modules()) == 1
        assert first.scale.dtype == first.shift.dtype == F32 and first.scale.shape == first.shift.shape == (32,)
        assert first.w_fwd.dtype == first.w_bwd.dtype == BF16 and first.w_fwd.shape == (32, 48) and first.w_bwd.shape == (3, 288)
        assert first.mean == [0.485, 0.456, 0.406] and first.inv_std == [1 / 0.229, 1 / 0.224, 1 / 0.225]
        assert sorted(_net(net).state_dict()) == sorted(_net(plain).state_dict()) == sorted(_net(off).state_dict())
        for a, b in zip(_net(off).state_dict().values(), _net(net).state_dict().values()):
            assert torch.equal(a, b)
    assert not any(isinstance(m, (zoo._OwnDepthwise, zoo._Pw8Tables)) for m in on.modules())
    assert sum(isinstance(m, zoo._OwnDepthwise) for m in all3.modules()) == 17
    assert sum(isinstance(m, zoo._Pw8Tables) for m in all3.modules()) == 34
    # off the GPU the rewritten network normalises in torch and runs its original modules: the same function, bit for bit
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(0))
    assert torch.equal(off(x.bfloat16()), on(x.bfloat16())) and torch.equal(off(x.bfloat16()), all3(x.bfloat16()))
    fp = zoo.build_classifier("mobilenet", num_classes=10, seed=1)
    zoo.use_own_first_conv_(fp[1], [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    assert torch.equal(plain(x), fp[1](x))
    # the tables: fp64-derived, fp32 whatever the cast, bit for bit; the packed weights are the weight's own rounding
    a, b = fp[1].features[0], on[0].features[0]
    scale, shift = zoo._bn_affine(a[1])
    assert torch.equal(a.scale, scale) and torch.equal(b.scale, scale) and torch.equal(b.shift, shift)
    assert torch.equal(b.w_fwd, a.w_fwd) and torch.equal(b.w_bwd, a.w_bwd)
    assert torch.equal(b.w_fwd.reshape(32, 3, 4, 4)[:, :, :3, :3].permute(0, 3, 1, 2), b[0].weight.detach())
    again = on.float().to(torch.bfloat16)
    assert again[0].features[0].scale.dtype == F32 and torch.equal(again[0].features[0].scale, scale)
    # a checkpoint saved from one variant loads into the other
    p_on, p_off = os.path.join(str(tmp_path), "on.pt"), os.path.join(str(tmp_path), "off.pt")
    torch.save(_net(on).state_dict(), p_on)
    torch.save(_net(plain).state_dict(), p_off)
    into_off = zoo.build_classifier("mobilenet", weights=p_on, **kw)
    into_on = zoo.build_classifier("mobilenet", weights=p_off, own_first_conv=True, **kw)
    assert torch.equal(into_off(x.bfloat16()), off(x.bfloat16())) and torch.equal(into_on(x.bfloat16()), off(x.bfloat16()))


def test_cli_flag_defaults_to_the_library():
    import demo_dL_attack
    p = demo_dL_attack.build_parser()
    a = p.parse_args([])
    assert a.own_first_conv == 0 and a.own_pointwise == 0 and a.own_depthwise == 0
    a = p.parse_args(["--own-first-conv", "1"])
    assert a.own_first_conv == 1 and a.own_pointwise == 0 and a.own_depthwise == 0
    a = p.parse_args(["--own-first-conv", "1", "--own-pointwise", "1", "--own-depthwise", "1"])
    assert (a.own_first_conv, a.own_pointwise, a.own_depthwise) == (1, 1, 1)
    with pytest.raises(SystemExit):
        p.parse_args(["--own-first-conv", "2"])
