"""CPU: host side of the VGG first-group kernels (adil_first3x3_pool_fwd / _bwd): the built library exports the symbols,
the header declares them and they refuse bad arguments without a device; the premises of the legs of
tests/vgg_first_reference.py on the reference alone; the fp32 emulation of the kernels' own accumulation order against
the fp64 reference on every row of the GPU table; the exact legs' power to reject mutants; the weight packs; the
`own_vgg_first_conv` switch, the CLI flag and the rewritten network on CPU inputs."""
import ctypes
import os
import re

import pytest
import torch

import vgg_first_reference as vf
from classifier_reference import BF16, F32, Arith

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"adil_first3x3_pool_fwd": 16, "adil_first3x3_pool_bwd": 12}


def test_library_exports_and_header_declares_the_new_symbols():
    from dl_attack_on_imagenet_amd import _lib
    from dl_attack_on_imagenet_amd.build import build_library
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIBPATH)
    src = open(os.path.join(ROOT, "include", "adil_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert name in src.split("int adil_abi_version")[0]            # the ABI comment's list of additive symbols
    bound = _lib.load()
    assert bound.adil_abi_version() == _lib.ABI_VERSION == 8
    # refusals need no device: they return before any HIP call
    f, b = bound.adil_first3x3_pool_fwd, bound.adil_first3x3_pool_bwd
    nm = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    fwd = lambda x, dt, w, bias, y, idx, B, H, W: f(x, dt, w, *nm, bias, y, idx, B, H, W, None)
    bwd = lambda g, idx, w, gx, dt, B, H, W: b(g, idx, w, *nm[3:], gx, dt, B, H, W, None)
    for (B, H, W, dt) in [(0, 8, 8, 0), (-1, 8, 8, 1), (1, 0, 8, 0), (1, 8, 0, 1), (1, 7, 8, 0), (1, 8, 7, 1), (1, 8, 8, 2),
                          (1, 8, 8, -1), (65536, 2, 2, 1), (2, 32768, 32768, 1)]:
        assert fwd(16, dt, 16, 16, 16, 16, B, H, W) == -1, (B, H, W, dt)
        assert bwd(16, 16, 16, 16, dt, B, H, W) == -1, (B, H, W, dt)
    for i in range(5):                                                 # each NULL pointer in turn
        a = [16] * 5
        a[i] = None
        assert fwd(a[0], 0, a[1], a[2], a[3], a[4], 1, 8, 8) == -1
    for i in range(4):
        a = [16] * 4
        a[i] = None
        assert bwd(a[0], a[1], a[2], a[3], 0, 1, 8, 8) == -1
    assert fwd(16, 0, 24, 16, 16, 16, 1, 8, 8) == -1                   # misaligned w_fwd
    assert fwd(16, 0, 16, 24, 16, 16, 1, 8, 8) == -1                   # misaligned bias
    assert fwd(16, 0, 16, 16, 24, 16, 1, 8, 8) == -1                   # misaligned y
    assert fwd(16, 0, 16, 16, 16, 24, 1, 8, 8) == -1                   # misaligned idx
    assert fwd(18, 0, 16, 16, 16, 16, 1, 8, 8) == -1                   # fp32 x on a 2-byte boundary
    assert fwd(17, 1, 16, 16, 16, 16, 1, 8, 8) == -1                   # bf16 x on an odd address
    assert bwd(24, 16, 16, 16, 0, 1, 8, 8) == -1                       # misaligned g
    assert bwd(16, 20, 16, 16, 0, 1, 8, 8) == -1                       # misaligned idx
    assert bwd(16, 16, 24, 16, 0, 1, 8, 8) == -1                       # misaligned w_bwd
    assert bwd(16, 16, 16, 18, 0, 1, 8, 8) == -1                       # fp32 gx on a 2-byte boundary
    assert bwd(16, 16, 16, 17, 1, 1, 8, 8) == -1                       # bf16 gx on an odd address


def test_kernels_compile_without_scratch():
    """What the compiler reports for the four instantiations (profiles/vgg_first_kernel_resources.md): no scratch, no
    spills, the LDS of the two tiles.  The backward's `__launch_bounds__(256, 2)` leaves the register allocator little
    room, so a compiler that starts to spill there is noticed here."""
    import subprocess
    from dl_attack_on_imagenet_amd import build
    src = os.path.join(build.CSRC, "adil_vgg_first.hip")
    r = subprocess.run([build._hipcc(), f"--offload-arch={build.ARCH}", "--cuda-device-only", "-O3", "-std=c++17", "-c", src, "-o",
                        os.devnull, "-I", os.path.join(ROOT, "include"), "-I", build.CSRC,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    kernels = {b.split()[0]: b for b in blocks if "first3x3_pool_" in b.split()[0]}
    assert len(kernels) == 4 and sum("pool_fwd" in k for k in kernels) == 2, sorted(kernels)
    field = lambda b, name: int(re.search(re.escape(name) + r":\s*(\d+)", b).group(1))
    for name, b in kernels.items():
        assert field(b, "ScratchSize [bytes/lane]") == 0 and field(b, "VGPRs Spill") == 0 and field(b, "SGPRs Spill") == 0, name
        assert field(b, "LDS Size [bytes/block]") == (5184 if "pool_fwd" in name else 78336), name
        assert field(b, "Occupancy [waves/SIMD]") >= (3 if "pool_fwd" in name else 2), name


def test_row_sets_hold_what_the_issue_lists():
    shapes = {r[:3] for r in vf.ROWS}
    assert {(1, 2, 2), (3, 6, 10), (2, 8, 8), (1, 2, 34), (1, 34, 2), (1, 224, 224)} <= shapes
    for th, tw in (vf.FWD_TILE, vf.BWD_TILE):
        assert {(1, h, w) for h in (th - 2, th, th + 2) for w in (tw - 2, tw, tw + 2)} <= shapes
        assert any(b > 1 and h > th and w > tw for b, h, w in shapes)
    assert {r[3] for r in vf.ROWS} == {BF16, F32} and len(set(vf.ROWS)) == len(vf.ROWS)
    assert vf.OOB_ROWS == [(1, 6, 10), (1, vf.FWD_TILE[0] + 2, vf.FWD_TILE[1] + 2)]
    assert all(r in vf.ROWS for r in vf.HASH_ROWS)


def _emu_fwd(emu, op):
    return vf.first_pool_fwd(emu, op.x, op.w, op.bias, op.mean, op.inv_std)


def _emu_bwd(emu, op, idx, dtype):
    return vf.finish_bwd(emu, vf.first_pool_bwd(emu, op.g, idx, op.w, op.inv_std, dtype))


@pytest.mark.parametrize("row", vf.ROWS, ids=str)
def test_emulation_passes_every_leg_and_the_premises_hold(row):
    """Every row of the GPU table with the kernel replaced by its fp32 emulation (one partial sum per MFMA, the kernel's
    own order): the premises on the reference alone (inside `exact_references` / `gaussian_references`), then bit for bit
    on the exact legs and under the bounds on the gaussian leg."""
    emu = Arith(F32, chunk=16)
    for leg in vf.EXACT_LEGS:
        name = vf.row_name(row, leg)
        r = vf.exact_references(row, leg)
        got = _emu_fwd(emu, r.op)
        vf.compare_fwd_exact(name, got.y, got.idx, r.fwd)
        vf.compare_bwd_exact(name, _emu_bwd(emu, r.op, r.fwd.idx, row[3]), r.bwd)
        print(name, r.shares)
    name = vf.row_name(row, "gaussian")
    g = vf.gaussian_references(row)
    got = _emu_fwd(emu, g.op)
    rf, undecided = vf.gaussian_fwd(name, got.y, got.idx, g)
    rb = vf.gaussian_bwd_ratio(_emu_bwd(emu, g.op, g.idx, row[3]), g.bwd)
    print(name, "max |err| / bound: fwd %.3f bwd %.3f; undecided windows %d of %d" % (rf, rb, undecided, g.idx.numel()))
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)


MUTANT_ROWS = [(3, 6, 10, F32), (2, 8, 8, BF16), (1, 18, 34, F32)]
FWD_MUTANTS = ["mean_sign", "raw_pad", "no_round_x", "chan_order", "last_winner", "bias_after_max", "dead_passes", "neg_zero",
               "trunc"]
BWD_MUTANTS = ["dead_passes_bwd", "flip_taps", "trunc"]


def _exact_legs(emu):
    """The exact legs of tests/test_gpu_vgg_first.py with the kernel replaced by the emulation `emu`; the names of the
    comparisons that failed, forward and gradient apart."""
    failed = {"fwd": [], "bwd": []}
    for row in MUTANT_ROWS:
        for leg in vf.EXACT_LEGS:
            name = vf.row_name(row, leg)
            r = vf.exact_references(row, leg)
            got = _emu_fwd(emu, r.op)
            for what, run in (("fwd", lambda: vf.compare_fwd_exact(name, got.y, got.idx, r.fwd)),
                              ("bwd", lambda: vf.compare_bwd_exact(name, _emu_bwd(emu, r.op, r.fwd.idx, row[3]), r.bwd))):
                try:
                    run()
                except AssertionError:
                    failed[what].append(name)
    return failed


def test_exact_legs_pass_the_emulation_and_reject_the_mutants():
    """Mean sign, padding in raw-pixel space, x' left unrounded, channel order, last winner instead of first, bias after
    the max, a dead window passing its gradient (as the forward's idx and as the gradient's reading of idx = 4), taps
    flipped in the gradient, -0 emitted, truncation for RNE: each is rejected where it acts; the emulation is not."""
    assert MUTANT_ROWS and all(r in vf.ROWS for r in MUTANT_ROWS)
    assert _exact_legs(Arith(F32, chunk=16)) == {"fwd": [], "bwd": []}
    for side, mutants in (("fwd", FWD_MUTANTS), ("bwd", BWD_MUTANTS)):
        for m in mutants:
            failed = _exact_legs(Arith(F32, chunk=16, mut=(m,)))[side]
            print(side, m, "rejected by", len(failed), "comparisons, e.g.", failed[:2])
            assert failed, "mutant %s passes the exact legs (%s)" % (m, side)


def test_pack_first3x3_pool_weights_round_trips_and_refuses_other_shapes():
    from dl_attack_on_imagenet_amd import ops
    w = torch.randn(64, 3, 3, 3, generator=torch.Generator().manual_seed(2))
    wf, wb = ops.pack_first3x3_pool_weights(w)
    assert wf.shape == (64, 48) and wb.shape == (3, 576) and wf.dtype == wb.dtype == BF16
    assert wf.is_contiguous() and wb.is_contiguous()
    wf4, wb3 = wf.reshape(64, 3, 4, 4), wb.reshape(3, 9, 64)
    assert torch.equal(wf4[:, :, :3, :3].permute(0, 3, 1, 2), w.bfloat16())          # [n][kh][kw][c] -> [n][c][kh][kw]
    assert bool((wf4[:, :, 3] == 0).all()) and bool((wf4[:, :, :, 3] == 0).all())
    assert torch.equal(wb3.reshape(3, 3, 3, 64).permute(3, 0, 1, 2), w.bfloat16())   # [c][kh][kw][n] -> [n][c][kh][kw]
    assert torch.equal(wf4, vf.pack_fwd(w.bfloat16())) and torch.equal(wb3, vf.pack_bwd(w.bfloat16()))
    for shape in [(32, 3, 3, 3), (64, 4, 3, 3), (64, 3, 7, 7), (64, 3, 3), (64, 27)]:
        with pytest.raises(ValueError):
            ops.pack_first3x3_pool_weights(torch.zeros(shape))
    x = torch.zeros(2, 3, 8, 8)
    assert not ops.first_conv3x3_pool_covers(x)                                      # not on a GPU
    with pytest.raises(ValueError):
        ops.first_conv3x3_pool(x, wf, wb, torch.zeros(64), (0, 0, 0), (1, 1, 1))


def test_switch_refusals_and_table():
    from dl_attack_on_imagenet_amd import zoo
    ok = dict(dtype=torch.bfloat16, channels_last=True, own_vgg_conv=True, own_vgg_first_conv=True, num_classes=8)
    with pytest.raises(ValueError, match="own_vgg_first_conv is a switch of VGG11"):
        zoo.build_classifier("mobilenet", **dict(ok, own_vgg_conv=False))
    with pytest.raises(ValueError, match="needs a bfloat16 network"):
        zoo.build_classifier("vgg11", **dict(ok, dtype=torch.float32))
    with pytest.raises(ValueError, match="needs channels_last=True"):
        zoo.build_classifier("vgg11", **dict(ok, channels_last=False))
    for bad in (dict(dtype=torch.float32), dict(channels_last=False)):   # the row's own conditions, behind the required switch's
        values = dict(own_vgg_conv=True, own_vgg_first_conv=True)
        with pytest.raises(ValueError, match="own_vgg_first_conv needs"):
            zoo._check_switch(zoo.VGG_FIRST_SWITCHES[0], values, "vgg11", bad.get("dtype", torch.bfloat16),
                              bad.get("channels_last", True))
    with pytest.raises(ValueError, match="own_vgg_first_conv needs own_vgg_conv=True"):
        zoo.build_classifier("vgg11", **dict(ok, own_vgg_conv=False))
    with pytest.raises(ValueError, match="own_vgg_conv"):
        zoo.use_own_vgg_first_conv_(zoo.build_classifier("vgg11", num_classes=8)[1], (0, 0, 0), (1, 1, 1))
    (row,) = zoo.VGG_FIRST_SWITCHES
    assert row.keyword == "own_vgg_first_conv" and row.flag == "--own-vgg-first-conv" and row.network == "vgg11"
    assert row.bf16 and row.channels_last and row.normalises and row.requires == ("own_vgg_conv",)
    assert row.keyword in zoo.build_classifier.__doc__ and row.help in zoo.build_classifier.__doc__
    assert row.keyword not in [r.keyword for r in zoo.SWITCHES + zoo.VGG_SWITCHES]


def _demo(argv):
    import demo_dL_attack
    args = demo_dL_attack.build_parser().parse_args(argv)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    return demo_dL_attack.classifier_keywords(args, args.model.lower(), dtype)


def test_cli_flag_and_keywords():
    """--own-vgg-first-conv defaults to 0 and refuses 2; its help names the flag it needs; the keyword is in the dictionary
    only when the flag is on, on vgg in bf16."""
    import demo_dL_attack
    p = demo_dL_attack.build_parser()
    assert p.parse_args([]).own_vgg_first_conv == 0 and p.parse_args(["--own-vgg-first-conv", "1"]).own_vgg_first_conv == 1
    with pytest.raises(SystemExit):
        p.parse_args(["--own-vgg-first-conv", "2"])
    (action,) = [a for a in p._actions if a.dest == "own_vgg_first_conv"]
    assert "needs --own-vgg-conv 1" in action.help
    both = ["--own-vgg-conv", "1", "--own-vgg-first-conv", "1"]
    on = _demo(["-m", "vgg", "--dtype", "bf16"] + both)
    assert on["own_vgg_first_conv"] is True and on["own_vgg_conv"] is True and on["channels_last"] is True
    assert _demo(["-m", "vgg", "--dtype", "bf16", "--own-vgg-conv", "1"]) == {k: v for k, v in on.items() if k != "own_vgg_first_conv"}
    for argv in (["-m", "vgg", "--dtype", "bf16"], ["-m", "vgg", "--dtype", "fp32"] + both, ["-m", "mobilenet", "--dtype", "bf16"] + both,
                 ["-m", "resnet50", "--dtype", "bf16"] + both):
        assert "own_vgg_first_conv" not in _demo(argv), argv


def test_switched_network_on_the_cpu():
    """A bf16 VGG11 built with both switches on the CPU: the Sequential holds the network alone, the network has the plain
    state-dict keys and loads the plain state dict, the new buffers are non-persistent under names of their own (the bias
    table fp32 through the cast, the packs the weight's own rounding), and on a CPU input, where the first group falls
    back, it equals Sequential(Normalize, plain) bit for bit at 32 x 32 and at an odd 33 x 33 (the smallest odd size that
    survives VGG11's five pools: 31 x 31 reaches the last pool as 1 x 1, which torch refuses in the plain network too)."""
    from dl_attack_on_imagenet_amd import ops, zoo
    kw = dict(num_classes=8, dtype=torch.bfloat16, channels_last=True)
    plain = zoo.build_classifier("vgg11", **kw)
    conv_only = zoo.build_classifier("vgg11", own_vgg_conv=True, **kw)
    own = zoo.build_classifier("vgg11", own_vgg_conv=True, own_vgg_first_conv=True, **kw)
    assert len(own) == 1 and isinstance(own[0], zoo.VGG11) and isinstance(plain[0], zoo.Normalize)
    feats = own[0].features
    assert isinstance(feats, zoo._OwnVggFeatures)
    sd0, sd1 = plain[1].state_dict(), own[0].state_dict()
    assert list(sd0) == list(sd1) and all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    own[0].load_state_dict(sd0)
    new = {"first_w_fwd", "first_w_bwd", "first_bias", "norm_mean", "norm_std"}
    assert set(feats._buffers) - set(conv_only[1].features._buffers) == new
    assert not new & set(conv_only[1].features._buffers)
    conv = feats._modules[feats._groups[0][0]]
    wf, wb = ops.pack_first3x3_pool_weights(conv.weight)
    assert torch.equal(feats.first_w_fwd, wf) and torch.equal(feats.first_w_bwd, wb) and wf.dtype == BF16
    assert feats.first_w_fwd.dim() == feats.first_w_bwd.dim() == 2
    assert feats.first_bias.dtype == F32 and torch.equal(feats.first_bias.bfloat16(), conv.bias)
    assert feats.mean == [0.485, 0.456, 0.406] and feats.inv_std == [1 / 0.229, 1 / 0.224, 1 / 0.225]
    again = own.float().to(torch.bfloat16)
    assert again[0].features.first_bias.dtype == F32 and torch.equal(again[0].features.first_bias, feats.first_bias)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for size in (32, 33):
            x = torch.rand(2, 3, size, size, generator=gen).bfloat16()
            want = plain(x)
            assert torch.equal(own(x), want) and torch.equal(conv_only(x), want), size
            xcl = x.contiguous(memory_format=torch.channels_last)
            assert torch.equal(own(xcl), plain(xcl)), size
