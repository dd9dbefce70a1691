"""CPU: the restatement of the pooled fp32 head kernels (tests/head_reference.py) against its own fp32 emulation and five
mutants, the premises of its exact leg, and the MobileNetV2 rewrite (`build_classifier(..., head_fp32=...)`, `zoo._OwnHead`)
on the CPU, where the module runs `_Fp32Head`'s torch formula."""
import os

import pytest
import torch
import torch.nn.functional as F

import head_reference as href
from classifier_reference import BF16, F32

MUTANTS = ("pooled_bf16", "trunc", "drop_last", "no_bias", "w_transposed")


@pytest.mark.parametrize("row", href.ROWS, ids=str)
def test_emulation_passes_both_legs(row):
    """The fp32 emulation of the kernels (their pixel order, 16-wide GEMM chunks) equals the exact leg's one correct value bit
    for bit and stays within the derived bounds of the gaussian leg."""
    name = href.row_name(row, "exact")
    op, want = href.exact_references(name, *row)
    href.compare_exact(name, href.emulate(op), want)
    name = href.row_name(row, "gaussian")
    op = href.operands(name, "gaussian", *row)
    ratios = href.gaussian_ratios(name, op, href.emulate(op))
    print(name, "max |err| / bound: pooled %.3f logits %.3f gpooled %.3f" % ratios)
    assert max(ratios) <= 1.0, (name, ratios)


@pytest.fixture(scope="module")
def exact_rows():
    return [(href.row_name(row, "exact"),) + href.exact_references(href.row_name(row, "exact"), *row) for row in href.ROWS]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_fails_an_exact_row(mutant, exact_rows):
    """pooled rounded to bf16, gx truncated instead of rounded to nearest even, the last pixel dropped, the bias omitted, w
    read transposed: each is caught by at least one row of the exact leg."""
    caught = []
    for name, op, want in exact_rows:
        try:
            href.compare_exact(name, href.emulate(op, (mutant,)), want)
        except AssertionError:
            caught.append(name)
    print(mutant, "caught by", len(caught), "of", len(exact_rows), "rows")
    assert caught, mutant


def test_pool_identity_premise():
    """f32(f32(HW k) * f32(1 / HW)) == k for HW in {9, 12, 25, 49, 100} and every integer and quarter-integer |k| <= 4096,
    and for every row's own HW on the k the exact leg draws (|k| <= 2)."""
    k = torch.arange(-4096 * 4, 4096 * 4 + 1, dtype=torch.float64) / 4
    for hw in href.IDENTITY_HW:
        href.assert_pool_identity("identity/%d" % hw, hw, k)
    small = torch.arange(-2, 3, dtype=torch.float64)
    for row in href.ROWS:
        if not href.is_pow2(row[1]):
            href.assert_pool_identity("identity/row/%d" % row[1], row[1], small)
    href.assert_pool_identity("identity/3136", 3136, small)             # the image of the 64-bit offset test
    with pytest.raises(AssertionError):                                  # the assertion can fail: 49 * 0.1 is not exact in fp32
        href.assert_pool_identity("identity/fails", 49, torch.tensor([0.1], dtype=torch.float64))


def test_rows_cover_the_contract():
    rows = href.ROWS
    for must in [(1, 1, 8, 1), (3, 49, 24, 10), (17, 9, 40, 7), (2, 16, 1280, 1000), (2, 4, 2048, 12), (67, 49, 64, 4)]:
        assert must in rows
    assert all(r in rows for r in href.NAN_ROWS)


# ------------------------------------------------------------------------------------------------------------- network
def _kw():
    return dict(num_classes=10, seed=3, dtype=BF16, channels_last=True)


def test_lib_declares_both_symbols():
    from dl_attack_on_imagenet_amd import _lib
    for name in ("adil_pool_head_fwd", "adil_pool_head_bwd"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["adil_pool_head_fwd"][1]) == 10 and len(_lib.SIGNATURES["adil_pool_head_bwd"][1]) == 9
    lib = _lib.load()                                                    # a library without them fails to load by name
    assert lib.adil_pool_head_fwd is not None and lib.adil_pool_head_bwd is not None
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "adil_hip.h")).read()
    assert "int adil_pool_head_fwd(" in header and "int adil_pool_head_bwd(" in header


def test_mobilenet_head_fp32_on_the_cpu(tmp_path):
    """head_fp32=True: fp32 logits equal to `_Fp32Head`'s formula on the network's own last activation; the state_dict keys
    of the plain network; a plain checkpoint loads; weight, bias and wt stay fp32, bit-identical, through casts."""
    from dl_attack_on_imagenet_amd import zoo
    plain = zoo.build_classifier("mobilenet", **_kw())
    path = os.path.join(str(tmp_path), "plain.pt")
    fp32_net = zoo.build_classifier("mobilenet", num_classes=10, seed=3)
    torch.save(fp32_net[-1].state_dict(), path)
    model = zoo.build_classifier("mobilenet", head_fp32=True, weights=path, **_kw())      # loads a plain checkpoint
    net = model[-1]
    assert isinstance(net.head32, zoo._OwnHead) and net.head32_on
    assert list(net.state_dict().keys()) == list(plain[-1].state_dict().keys())
    assert list(model.state_dict().keys()) == list(plain.state_dict().keys())
    net.load_state_dict(torch.load(path))                                # and again, strictly, after the rewrite
    fc = fp32_net[-1].classifier[-1]
    head = net.head32
    assert torch.equal(head.weight, fc.weight) and torch.equal(head.bias, fc.bias) and torch.equal(head.wt, fc.weight.t())
    assert head.wt.is_contiguous() and tuple(head.wt.shape) == (1280, 10)
    assert net.classifier[-1].weight.dtype == BF16
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(BF16)
    seen = []
    handle = net.features.register_forward_hook(lambda m, a, out: seen.append(out.detach()))
    logits = model(x)
    handle.remove()
    assert logits.dtype == F32 and logits.shape == (2, 10) and len(seen) == 1 and seen[0].dtype == BF16
    want = F.linear(seen[0].float().mean(dim=(2, 3)), fc.weight, fc.bias)
    assert torch.equal(logits, want)
    assert plain(x).dtype == BF16
    want_bits = {n: getattr(head, n).clone() for n in ("weight", "bias", "wt")}
    for cast in (lambda m: m.to(BF16), lambda m: m.float().to(BF16), lambda m: m.to(memory_format=torch.channels_last)):
        model = cast(model)
        for n, t in want_bits.items():
            got = getattr(model[-1].head32, n)
            assert got.dtype == F32 and torch.equal(got, t), n
    assert not any(isinstance(m, zoo._OwnHead) for m in plain.modules())
    three = zoo.build_classifier("mobilenet", own_depthwise=True, own_pointwise=True, own_first_conv=True, **_kw())
    assert not any(isinstance(m, zoo._Fp32Head) for m in three.modules()) and three[-1].head32 is None


def test_inference_mode_toggles_and_restores():
    from dl_attack_on_imagenet_amd import engine, zoo
    model = zoo.build_classifier("mobilenet", head_fp32="inference", **_kw())
    net = model[-1]
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(2)).to(BF16)
    assert net.head32 is not None and not net.head32_on and model(x).dtype == BF16
    with engine.precise_head(model):
        assert net.head32_on and model(x).dtype == F32
        with engine.precise_head(model, False):
            assert not net.head32_on and model(x).dtype == BF16
        assert net.head32_on and model(x).dtype == F32
    assert not net.head32_on and model(x).dtype == BF16
    try:
        with engine.precise_head(model):
            raise RuntimeError("x")
    except RuntimeError:
        pass
    assert not net.head32_on
    plain = zoo.build_classifier("mobilenet", **_kw())[-1]
    assert plain.head32 is None and plain.precise_head(True) is False and not plain.head32_on


def test_head_fp32_value_errors():
    from dl_attack_on_imagenet_amd import zoo
    for name in ("vgg11", "densenet121", "resnet18"):                    # other networks without the fused path: as before
        with pytest.raises(ValueError):
            zoo.build_classifier(name, num_classes=10, head_fp32=True, dtype=BF16, channels_last=True)
    with pytest.raises(ValueError):                                      # an fp32 network
        zoo.build_classifier("mobilenet", num_classes=10, head_fp32=True, channels_last=True)
    with pytest.raises(ValueError):                                      # not channels_last
        zoo.build_classifier("mobilenet", num_classes=10, head_fp32=True, dtype=BF16)
    with pytest.raises(ValueError):                                      # a bad mode
        zoo.build_classifier("mobilenet", num_classes=10, head_fp32="sometimes", dtype=BF16, channels_last=True)
    with pytest.raises(ValueError):
        zoo.use_own_head_(zoo.MobileNetV2(10), "sometimes")
    with pytest.raises(ValueError):
        zoo.use_own_head_(zoo._BUILDERS["resnet18"](10), True)
