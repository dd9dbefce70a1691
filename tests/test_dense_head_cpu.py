"""CPU: the restatement of the BatchNorm + ReLU pooled head kernels (tests/dense_head_reference.py) against its own fp32
emulation and eleven mutants, the premises of its exact leg, the bindings, and the DenseNet rewrite
(`build_classifier(..., own_dense_head=...)`, `zoo._OwnDenseHead`) on the CPU, where the module runs the torch formula."""
import os

import pytest
import torch
import torch.nn.functional as F

import dense_head_reference as dref
import head_reference as href
from classifier_reference import BF16, F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Mutants that no BIT-EXACT comparison of these rows can see, with the reason; what does reject them is asserted below.
EQUIVALENT = {
    "pre_bf16": "the exact leg's p are integers <= 8, which are bf16 values, and gx depends on the sign of pre alone; the "
                "gaussian leg's bound on pooled rejects it (2^-9 relative against HW 2^-23)",
    "scale_before_inv_hw": "with a power-of-two pscale (exact leg) or HW both orders give the same fp32 bits; elsewhere they "
                           "differ in the last fp32 bit of v for a part of the values, which the rounding to bf16 hides unless "
                           "v lies within 2^-16 of a tie: none of the 2e4 values of the gaussian rows does",
}
POOLED_BOUND_REJECTS = ("pre_bf16",)


@pytest.mark.parametrize("row", dref.ROWS, ids=str)
def test_emulation_passes_both_legs(row):
    """The fp32 emulation of the kernels (their pixel order, 16-wide GEMM chunks, the two roundings of the prologue) equals
    the exact leg's one correct value bit for bit and stays within the derived bounds of the gaussian leg."""
    name = dref.row_name(row, "exact")
    op, want = dref.exact_references(name, *row)
    dref.compare_exact(name, dref.emulate(op), want)
    name = dref.row_name(row, "gaussian")
    op = dref.operands(name, "gaussian", *row)
    ratios = dref.gaussian_ratios(name, op, dref.emulate(op))
    print(name, "max |err| / bound: pooled %.3f logits %.3f gpooled %.3f" % ratios)
    assert max(ratios) <= 1.0, (name, ratios)


@pytest.fixture(scope="module")
def rows():
    """Per row: the exact leg's operands and values, the gaussian leg's operands.  Computed once, never modified."""
    out = []
    for row in dref.ROWS:
        ne, ng = dref.row_name(row, "exact"), dref.row_name(row, "gaussian")
        out.append((ne,) + dref.exact_references(ne, *row) + (ng, dref.operands(ng, "gaussian", *row)))
    return out


@pytest.mark.parametrize("mutant", dref.MUTANTS)
def test_every_mutant_fails_a_bit_exact_comparison(mutant, rows):
    """Each mutant is rejected by a bit-for-bit comparison of some row: the four outputs of the exact leg, or the gaussian
    leg's gx (restated from the mutant's own gpooled).  `EQUIVALENT` pins the ones that are not, with what rejects them."""
    caught, worst_pooled = [], 0.0
    for ne, ope, want, ng, opg in rows:
        try:
            dref.compare_exact(ne, dref.emulate(ope, (mutant,)), want)
        except AssertionError:
            caught.append(ne)
        try:
            worst_pooled = max(worst_pooled, dref.gaussian_ratios(ng, opg, dref.emulate(opg, (mutant,)))[0])
        except AssertionError:
            caught.append(ng)
    print(mutant, "caught bit for bit by", len(caught), "of", 2 * len(rows), "comparisons; gaussian pooled ratio %.3g" % worst_pooled)
    if mutant in EQUIVALENT:
        assert not caught, (mutant, caught)
        assert (worst_pooled > 1.0) == (mutant in POOLED_BOUND_REJECTS), (mutant, worst_pooled)
    else:
        assert caught, mutant


def test_fma_flips_the_branch_in_the_zero_channels():
    """The gaussian leg's channels c % 8 == 3: pre is exactly 0 where x = +c_k, and one fma leaves a residual of both signs."""
    op = dref.operands("zero-channels", "gaussian", 3, 49, 24, 10)
    pre = dref.pre_of(dref.Arith(), op.x, op.pscale, op.pshift)[:, :, dref.ZERO_CHANNEL::8]
    fma = dref.pre_of(dref.Arith(mut=("fma",)), op.x, op.pscale, op.pshift)[:, :, dref.ZERO_CHANNEL::8]
    at = op.x[:, :, dref.ZERO_CHANNEL::8].float() > 0
    assert bool(at.any()) and bool((pre[at] == 0).all()) and bool((fma[at] != 0).any())
    assert bool((pre[~at] != 0).all())


def test_the_order_of_the_two_gradient_products_is_visible_in_fp32():
    """Why `scale_before_inv_hw` is specified although no row sees it through bf16: f32(f32(g / HW) s) and f32(f32(g s) / HW)
    differ in fp32 for a part of the values at HW = 49, and never for a power-of-two HW."""
    gen = torch.Generator().manual_seed(7)
    g, s = torch.randn(1, 4096, generator=gen), (0.5 + torch.rand(4096, generator=gen))
    for hw, differs in ((49, True), (16, False)):
        a = href.scale_f32(g, hw) * s
        b = href.scale_f32(g * s, hw)
        assert bool((a != b).any()) == differs, hw


def test_rows_cover_the_contract():
    assert all(r in dref.ROWS for r in href.ROWS)
    assert (2, 4, 1024, 1000) in dref.ROWS and (2, 49, 1024, 12) in dref.ROWS
    assert dref.NAN_ROWS == [(3, 49, 24, 10), (17, 9, 40, 7)] and all(r in dref.ROWS for r in dref.NAN_ROWS)
    hws = {r[1] for r in dref.ROWS}
    assert any(href.is_pow2(h) and h >= 64 for h in hws) and any(not href.is_pow2(h) and h % 2 == 1 for h in hws)
    assert any(h < 8 for h in hws) and any(h > 32 and h % 32 for h in hws)       # idle pixel rows; the 4-deep loop and its tail
    small = torch.arange(2, 5, dtype=torch.float64)
    for h in hws:
        if not href.is_pow2(h):
            href.assert_pool_identity("identity/row/%d" % h, h, small)


def test_lib_and_header_declare_both_symbols():
    from dl_attack_on_imagenet_amd import _lib
    for name in ("adil_bn_pool_head_fwd", "adil_bn_pool_head_bwd"):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 12
    lib = _lib.load()                                                    # a library without them fails to load by name
    assert lib.adil_bn_pool_head_fwd is not None and lib.adil_bn_pool_head_bwd is not None
    assert lib.adil_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "adil_hip.h")).read()
    assert "int adil_bn_pool_head_fwd(" in header and "int adil_bn_pool_head_bwd(" in header


# ------------------------------------------------------------------------------------------------------------- network
def _kw():
    return dict(num_classes=10, seed=3, dtype=BF16, channels_last=True)


def _formula(head, x):
    pre = x.float() * head.pscale.reshape(1, -1, 1, 1) + head.pshift.reshape(1, -1, 1, 1)
    return F.linear(F.relu(pre).mean((2, 3)), head.weight, head.bias)


def test_densenet_own_dense_head_on_the_cpu(tmp_path):
    """own_dense_head=True: fp32 logits equal to the torch formula on the head's own input; the state_dict keys of the plain
    network; a plain checkpoint loads before and after the rewrite; the five buffers stay fp32, bit-identical, through casts."""
    from dl_attack_on_imagenet_amd import zoo
    plain = zoo.build_classifier("densenet121", **_kw())
    path = os.path.join(str(tmp_path), "plain.pt")
    fp32_net = zoo.build_classifier("densenet121", num_classes=10, seed=3)
    with torch.no_grad():                                                # a norm5 that is no identity
        gen = torch.Generator().manual_seed(4)
        bn = fp32_net[-1].features.norm5
        bn.weight.copy_((0.7 + 0.6 * torch.rand(1024, generator=gen)) * (torch.randint(0, 2, (1024,), generator=gen) * 2 - 1))
        bn.bias.copy_(0.2 * torch.randn(1024, generator=gen))
        bn.running_mean.copy_(0.2 * torch.randn(1024, generator=gen))
        bn.running_var.copy_(0.6 + 0.8 * torch.rand(1024, generator=gen))
    torch.save(fp32_net[-1].state_dict(), path)
    model = zoo.build_classifier("densenet121", own_dense_head=True, weights=path, **_kw())     # loads a plain checkpoint
    net = model[-1]
    head = net.head32
    assert isinstance(head, zoo._OwnDenseHead) and net.head32_on
    assert isinstance(net.features.norm5, torch.nn.BatchNorm2d) and isinstance(net.classifier, torch.nn.Linear)
    assert list(net.state_dict().keys()) == list(plain[-1].state_dict().keys())
    assert list(model.state_dict().keys()) == list(plain.state_dict().keys())
    net.load_state_dict(torch.load(path))                                # and again, strictly, after the rewrite
    fc = fp32_net[-1].classifier
    pscale, pshift = zoo._bn_affine(fp32_net[-1].features.norm5)
    assert torch.equal(head.weight, fc.weight) and torch.equal(head.bias, fc.bias) and torch.equal(head.wt, fc.weight.t())
    assert torch.equal(head.pscale, pscale) and torch.equal(head.pshift, pshift) and bool((pscale < 0).any())
    assert head.wt.is_contiguous() and tuple(head.wt.shape) == (1024, 10)
    assert net.classifier.weight.dtype == BF16 and net.features.norm5.weight.dtype == BF16
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(BF16)
    seen = []
    handle = head.register_forward_pre_hook(lambda m, args: seen.append(args[0].detach()))
    logits = model(x)
    handle.remove()
    assert logits.dtype == F32 and logits.shape == (2, 10) and len(seen) == 1
    assert seen[0].dtype == BF16 and tuple(seen[0].shape) == (2, 1024, 2, 2)
    assert torch.equal(logits, _formula(head, seen[0]))
    assert plain(x).dtype == BF16
    want_bits = {n: getattr(head, n).clone() for n in ("weight", "bias", "wt", "pscale", "pshift")}
    for cast in (lambda m: m.to(BF16), lambda m: m.float().to(BF16), lambda m: m.to(memory_format=torch.channels_last)):
        model = cast(model)
        for n, t in want_bits.items():
            got = getattr(model[-1].head32, n)
            assert got.dtype == F32 and torch.equal(got, t), n
    assert not any(isinstance(m, zoo._Fp32Head) for m in plain.modules())
    # the trunk in front of the head is the plain network's: its norm5 sees the head's input
    twin = zoo.build_classifier("densenet121", weights=path, **_kw())
    got = []
    handle = twin[-1].features.norm5.register_forward_pre_hook(lambda m, args: got.append(args[0].detach()))
    twin(x)
    handle.remove()
    assert torch.equal(got[0], seen[0])


def test_inference_mode_toggles_and_restores():
    from dl_attack_on_imagenet_amd import engine, zoo
    model = zoo.build_classifier("densenet121", own_dense_head="inference", **_kw())
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
    plain = zoo.build_classifier("densenet121", **_kw())[-1]
    assert plain.head32 is None and plain.precise_head(True) is False and not plain.head32_on


def test_own_dense_head_value_errors():
    from dl_attack_on_imagenet_amd import zoo
    for name in ("mobilenet", "resnet18", "vgg11"):                      # another network
        with pytest.raises(ValueError):
            zoo.build_classifier(name, num_classes=10, own_dense_head=True, dtype=BF16, channels_last=True)
    with pytest.raises(ValueError):                                      # an fp32 network
        zoo.build_classifier("densenet121", num_classes=10, own_dense_head=True, channels_last=True)
    with pytest.raises(ValueError):                                      # not channels_last
        zoo.build_classifier("densenet121", num_classes=10, own_dense_head=True, dtype=BF16)
    with pytest.raises(ValueError):                                      # a bad mode
        zoo.build_classifier("densenet121", num_classes=10, own_dense_head="sometimes", dtype=BF16, channels_last=True)
    with pytest.raises(ValueError):
        zoo.use_own_dense_head_(zoo.DenseNet(num_classes=10), "sometimes")
    with pytest.raises(ValueError):
        zoo.use_own_dense_head_(zoo._BUILDERS["resnet18"](10), True)
    with pytest.raises(ValueError):                                      # head_fp32 stays a switch of the other networks
        zoo.build_classifier("densenet121", num_classes=10, head_fp32=True, dtype=BF16, channels_last=True)
