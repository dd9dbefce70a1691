"""CPU: host side of the strided dense kernels (adil_dense1x1_fwd_ld / _bwd_ld, adil_dense3x3_fwd_ld / _bwd_ld) and of the
dense-block path built on them: the built library exports the symbols, the header and the binding declare them, the
refusals return before any device call; the restatement of `accumulate = 1` (tests/dense_block_reference.py) with the
fp32 emulation of the kernel on both legs for every row of the GPU table and the premises asserted on the reference alone;
the comparators' power to reject the mutants of the accumulate rule; `_OwnDenseBlock`, the `own_dense_block` switch and
the CLI default."""
import copy
import ctypes
import os
import re

import pytest
import torch

import dense1x1_reference as d1
import dense3x3_reference as d3
import dense_block_reference as db
from classifier_reference import Arith, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 4096                       # a pitch that passes every ld test: the refusal under test is the one that answers


def test_library_exports_and_header_declares_the_new_symbols():
    from dl_attack_on_imagenet_amd import _lib
    from dl_attack_on_imagenet_amd.build import build_library
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIBPATH)
    src = open(os.path.join(ROOT, "include", "adil_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in db.NEW_SYMBOLS.items():
        assert hasattr(lib, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.load().adil_abi_version() == _lib.ABI_VERSION == 8


def _f1(lib):
    """adil_dense1x1_fwd_ld with the argument list of adil_dense1x1_fwd plus (ldx, ldy)."""
    return lambda x, ps, pb, w, sc, sh, y, m, k, n, act, st, ldx=BIG, ldy=BIG: lib.adil_dense1x1_fwd_ld(
        x, ldx, ps, pb, w, sc, sh, y, ldy, m, k, n, act, st)


def _b1(lib):
    """adil_dense1x1_bwd_ld with the argument list of adil_dense1x1_bwd plus (ldg, ldy, ldxin, ldgx, accumulate)."""
    return lambda g, y, sc, wt, xin, ps, pb, gx, m, k, n, act, st, ldg=BIG, ldy=BIG, ldxin=BIG, ldgx=BIG, acc=0: \
        lib.adil_dense1x1_bwd_ld(g, ldg, y, ldy, sc, wt, xin, ldxin, ps, pb, gx, ldgx, acc, m, k, n, act, st)


def test_dense1x1_ld_refusals_need_no_device():
    """Every refusal tests/test_dense1x1_cpu.py lists, through the _ld entries; then each ld below its width, each ld that
    is no multiple of 8, accumulate 2 and -1.  All return ADIL_EINVAL before any HIP call."""
    from dl_attack_on_imagenet_amd import _lib
    lib = _lib.load()
    f, b = _f1(lib), _b1(lib)
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
    fa, ba = (16,) * 7 + (8, 64, 32, 1, None), (16,) * 8 + (8, 64, 32, 1, None)      # M = 8, K = 64, N = 32
    for name, width in (("ldx", 64), ("ldy", 32)):
        for ld in (width - 8, width + 4, width + 1, 0, -width):
            assert f(*fa, **{name: ld}) == -1, (name, ld)
    for name, width in (("ldg", 32), ("ldy", 32), ("ldxin", 64), ("ldgx", 64)):
        for ld in (width - 8, width + 4, width + 1, 0, -width):
            assert b(*ba, **{name: ld}) == -1, (name, ld)
    for acc in (2, -1):
        assert b(*ba, acc=acc) == -1, acc


def test_dense3x3_ld_refusals_need_no_device():
    """Every refusal tests/test_dense3x3_cpu.py lists, through the _ld entries; then each ld below its width and each ld
    that is no multiple of 8."""
    from dl_attack_on_imagenet_amd import _lib
    lib = _lib.load()
    # (name, input-side width of (C, N), output-side width)
    for raw, win, wout in ((lib.adil_dense3x3_fwd_ld, 0, 1), (lib.adil_dense3x3_bwd_ld, 1, 0)):
        f = lambda s, wp, out, B, H, W, C, N, st, ldi=BIG, ldo=BIG: raw(s, ldi, wp, out, ldo, B, H, W, C, N, st)
        for dims in d3.REFUSED_DIMS:
            assert f(16, 16, 16, *dims, None) == -1, dims
        for i in range(3):
            null, odd = [16, 16, 16], [16, 16, 16]
            null[i], odd[i] = None, 24
            assert f(*null, 2, 4, 4, 32, 32, None) == -1, i        # each NULL pointer
            assert f(*odd, 2, 4, 4, 32, 32, None) == -1, i         # each misaligned pointer
        assert f(16, 16, 16, 2 ** 20, 2 ** 11, 1, 32, 32, None) == -1     # B H W = 2^31
        assert f(16, 16, 16, 2 ** 30, 2 ** 30, 63, 32, 32, None) == -1    # B H alone beyond 64-bit comfort
        cn = (64, 32)
        for name, width in (("ldi", cn[win]), ("ldo", cn[wout])):
            for ld in (width - 8, width - 32, width + 4, width + 1, 0, -width):
                assert f(16, 16, 16, 2, 4, 4, *cn, None, **{name: ld}) == -1, (name, ld)


@pytest.mark.parametrize("row", db.D1_LD_ROWS, ids=str)
def test_accumulate_emulation_passes_every_row(row):
    """The fp32 emulation of accumulate = 1 (one fp32 product, one fp32 add, one rounding; reduction in chunks of 16) equals
    the restatement bit for bit on the row's exact leg and stays under the gaussian bound.  On the reference alone, inside
    `reference_row`: the quantum and sum |terms| < 2^23 quanta with |old| included; here: the old -0.0 of the first row
    gives +0 wherever the element is masked."""
    name = db.row_name(*row)
    leg = db.exact_leg(row[3])
    (r, old, acc), got = db.emulate_accumulate(row, leg)
    d1.assert_premise(name + "/acc", acc, "clamp")               # the rounding share is asserted in its own test
    d1.compare_exact(name + "/acc", got, acc)
    want = d1.finish(Arith(), acc)
    masked = ~r.bwd.keep[0, ::2]
    assert bool((bits(old[0, ::2]) == -32768).all())
    assert bool((bits(want[0, ::2])[masked] == 0).all())         # -0.0 + (+0) = +0
    (r, old, acc), got = db.emulate_accumulate(row, "gaussian")
    ratio = d1.gaussian_ratio(got, acc)
    assert ratio <= 1.0, (name, ratio)


ROUNDING_ROWS = [r for r in db.D1_LD_ROWS if r[3] == 0]
CLAMP_ROWS = [r for r in db.D1_LD_ROWS if r[3] == 1 and r[0] > 1]


def _rejected(row, leg, mut):
    (r, old, acc), got = db.emulate_accumulate(row, leg, (mut,))
    if leg == "gaussian":
        return d1.gaussian_ratio(got, acc) > 1.0
    try:
        d1.compare_exact(mut, got, acc)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("row", ROUNDING_ROWS, ids=str)
def test_double_rounding_is_rejected(row):
    """Mutant (a): v rounded to bf16 before the add.  On the reference alone: with |old| <= OLD_AMP['rounding'] single and
    double rounding differ in at least 1 % of the rounding set's outputs; the emulation with the mutant fails
    compare_exact, without it passes."""
    assert len(ROUNDING_ROWS) == 2
    r, old, acc = db.reference_row(row, "rounding")
    ref = Arith()
    one = d1.finish(ref, acc)
    two = d1.finish(ref, db.accumulate(ref, r.bwd, old, ("double_round",)))
    share = float((bits(one) != bits(two)).double().mean())
    assert share >= 0.01, (row, share)
    assert _rejected(row, "rounding", "double_round")
    assert not _rejected(row, "rounding", "none")


@pytest.mark.parametrize("mut", ["ignored", "no_mask", "row_old"])
@pytest.mark.parametrize("row,leg", [(r, "rounding") for r in ROUNDING_ROWS[:1]] + [(r, "clamp") for r in CLAMP_ROWS[:2]]
                         + [(CLAMP_ROWS[0], "gaussian")], ids=str)
def test_comparators_reject_the_accumulate_mutants(mut, row, leg):
    """Mutants (b) accumulate ignored, (c) the mask dropped on the added value, (d) the old value of the neighbouring row:
    none passes the exact leg; the gaussian leg rejects them too; the unmutated emulation passes."""
    assert _rejected(row, leg, mut), (mut, row, leg)
    assert not _rejected(row, leg, "none")


# ----------------------------------------------------------------------------------------------------------- the switch
def _randomise_bn(net, seed=1):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=gen))
                m.running_var.copy_(0.6 + 0.8 * torch.rand(m.num_features, generator=gen))
                m.weight.copy_(torch.randn(m.num_features, generator=gen))


def test_rewrite_keeps_the_function_and_the_state_dict():
    """use_own_dense_block_ rewrites the 4 blocks of a network that both other rewrites have been through and nothing on
    one that has not; the state_dict keys and values stay, and on a CPU fp32 input the rewritten network IS the plain
    network, bit for bit (the fallback loop); the block holds the very layer objects, no copies of their tables."""
    from dl_attack_on_imagenet_amd import zoo
    torch.manual_seed(0)
    plain = zoo.DenseNet(num_classes=16).eval()
    _randomise_bn(plain)
    own = copy.deepcopy(plain)
    assert zoo.use_own_dense_block_(own) == 0                      # plain layers: nothing to take over
    assert zoo.use_own_dense_pointwise_(own) == 61
    assert zoo.use_own_dense_block_(own) == 0                      # library growth convolutions: still nothing
    assert zoo.use_own_dense_conv_(own) == 58
    layer = own.features.denseblock2.denselayer3
    assert zoo.use_own_dense_block_(own) == 4
    assert zoo.use_own_dense_block_(own) == 0
    blocks = [m for m in own.modules() if isinstance(m, zoo._OwnDenseBlock)]
    assert [len(b) for b in blocks] == [6, 12, 24, 16]
    assert own.features.denseblock2.denselayer3 is layer
    assert not list(blocks[0].named_buffers(recurse=False)) and not list(blocks[0].named_parameters(recurse=False))
    sd0, sd1 = plain.state_dict(), own.state_dict()
    assert list(sd0.keys()) == list(sd1.keys())
    assert all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    plain.load_state_dict(sd1)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        assert torch.equal(plain(x), own(x))
    with pytest.raises(ValueError):
        zoo._OwnDenseBlock(zoo._DenseBlock(2, 64))                 # plain children
    mixed = copy.deepcopy(blocks[0])
    mixed._modules["denselayer2"] = copy.deepcopy(blocks[1].denselayer1)      # input widths no longer consecutive
    assert not zoo._is_own_dense_block(mixed)


def test_build_classifier_switch():
    """own_dense_block needs DenseNet-121 and both other switches (hence bf16 and channels_last); with them 4 blocks are
    rewritten and the state_dict keys are the plain network's; off by default."""
    from dl_attack_on_imagenet_amd import zoo
    ok = dict(dtype=torch.bfloat16, channels_last=True, own_dense_pointwise=True, own_dense_conv=True, own_dense_block=True,
              num_classes=8)
    with pytest.raises(ValueError, match="own_dense_block is a switch of DenseNet-121"):
        zoo.build_classifier("resnet18", dtype=torch.bfloat16, channels_last=True, own_dense_block=True, num_classes=8)
    with pytest.raises(ValueError, match="own_dense_block needs own_dense_pointwise=True and own_dense_conv=True"):
        zoo.build_classifier("densenet121", **dict(ok, own_dense_pointwise=False))
    with pytest.raises(ValueError, match="own_dense_block needs own_dense_pointwise=True and own_dense_conv=True"):
        zoo.build_classifier("densenet121", **dict(ok, own_dense_conv=False))
    with pytest.raises(ValueError, match="needs a bfloat16 network"):
        zoo.build_classifier("densenet121", **dict(ok, dtype=torch.float32))
    with pytest.raises(ValueError, match="needs channels_last=True"):
        zoo.build_classifier("densenet121", **dict(ok, channels_last=False))
    model = zoo.build_classifier("densenet", **ok)
    assert sum(isinstance(m, zoo._OwnDenseBlock) for m in model.modules()) == 4
    assert sum(isinstance(m, zoo._OwnDenseLayer) for m in model.modules()) == 58
    assert sum(isinstance(m, zoo._OwnGrowthConv) for m in model.modules()) == 58
    plain = zoo.build_classifier("densenet", num_classes=8)
    assert list(model.state_dict().keys()) == list(plain.state_dict().keys())
    two = zoo.build_classifier("densenet", **dict(ok, own_dense_block=False))
    assert not any(isinstance(m, zoo._OwnDenseBlock) for m in two.modules())
    with torch.no_grad():                                          # a CPU input takes the loop over the children
        x = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(3)).bfloat16()
        assert torch.equal(model(x), two(x))


def test_dense_block_covers_and_validation():
    """ops.dense_block_covers on CPU tensors and shapes (no device needed): CUDA only, bf16, the widths of both kernel
    families, W <= 63; ops.dense_block refuses an uncovered input and malformed layer tuples with ValueError."""
    from dl_attack_on_imagenet_amd import ops
    x = torch.zeros(1, 64, 4, 4, dtype=torch.bfloat16)
    assert not ops.dense_block_covers(x, 64, 6, 32, 128)           # not on the GPU
    with pytest.raises(ValueError):
        ops.dense_block(x, [])
    with pytest.raises(ValueError):
        ops.dense_block(x, [(x,) * 7])
    t = lambda *s: torch.zeros(*s)
    layer = (t(64), t(64), t(128, 64).bfloat16(), t(64, 128).bfloat16(), t(128), t(128), t(32, 9 * 128).bfloat16(),
             t(128, 9 * 32).bfloat16())
    with pytest.raises(ValueError, match="do not cover"):
        ops.dense_block(x, [layer])


def test_cli_switches_default_to_off():
    import demo_dL_attack
    import main
    for mod in (demo_dL_attack, main):
        p = mod.build_parser()
        assert p.parse_args([]).own_dense_block == 0
        assert p.parse_args(["--own-dense-block", "1"]).own_dense_block == 1
