"""CPU: host side of the depthwise 3x3 kernels (adil_dw3x3_fwd / adil_dw3x3_bwd): the built library exports the symbols
and the header declares them, the BatchNorm-folded weight packing against the fp64 fold, the fp64 restatement of
tests/depthwise_reference.py against torch's grouped convolution and its autograd, the exact leg's power to reject
mutants (run on the fp32 emulation of the kernel), the `own_depthwise` switch and the CLI default."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import depthwise_reference as dref
from classifier_reference import F32, F64, Arith

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adil_dw3x3_fwd", "adil_dw3x3_bwd")


def test_library_exports_and_header_declares_the_new_symbols():
    from dl_attack_on_imagenet_amd import _lib
    from dl_attack_on_imagenet_amd.build import build_library
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIBPATH)
    src = open(os.path.join(ROOT, "include", "adil_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 11
    bound = _lib.load()
    assert bound.adil_abi_version() == _lib.ABI_VERSION == 8
    # refusals need no device: they return before any HIP call
    for fn in (bound.adil_dw3x3_fwd, bound.adil_dw3x3_bwd):
        assert fn(None, None, None, None, 1, 8, 8, 8, 1, 1, None) == -1
        assert fn(16, 16, 16, 16, 1, 8, 8, 12, 1, 1, None) == -1
        assert fn(16, 16, 16, 16, 1, 8, 8, 8, 3, 1, None) == -1
        assert fn(16, 16, 16, 16, 0, 8, 8, 8, 1, 1, None) == -1


def test_packing_equals_the_fp64_fold():
    from dl_attack_on_imagenet_amd import ops, zoo
    gen = torch.Generator().manual_seed(5)
    C = 24
    conv = torch.nn.Conv2d(C, C, 3, 1, 1, groups=C, bias=False)
    bn = torch.nn.BatchNorm2d(C).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(C, 1, 3, 3, generator=gen))
        bn.weight.copy_(torch.randn(C, generator=gen))                  # both signs, as in pretrained networks
        bn.bias.copy_(torch.randn(C, generator=gen))
        bn.running_mean.copy_(torch.randn(C, generator=gen))
        bn.running_var.copy_(torch.rand(C, generator=gen) + 0.1)
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    w9c = ops.pack_dw3x3_weights(conv.weight, scale)
    assert w9c.shape == (9, C) and w9c.dtype == torch.float32 and w9c.is_contiguous()
    want = (conv.weight.detach().double() * scale.view(C, 1, 1, 1)).float()          # [c][0][kh][kw]
    for kh in range(3):
        for kw in range(3):
            assert torch.equal(w9c[kh * 3 + kw], want[:, 0, kh, kw])
    assert torch.equal(ops.pack_dw3x3_weights(conv.weight), conv.weight.detach().reshape(C, 9).t())
    block = zoo._ConvBNReLU6(C, C, 3, 1, C).eval()
    block[0].load_state_dict(conv.state_dict())
    block[1].load_state_dict(bn.state_dict())
    own = zoo._OwnDepthwise(block)
    assert torch.equal(own.w9c, w9c)
    assert torch.equal(own.bias, (bn.bias.detach().double() - bn.running_mean.double() * scale).float())
    for bad in (torch.zeros(C, C, 3, 3), torch.zeros(C, 1, 1, 1), torch.zeros(C, 2, 3, 3), torch.zeros(C, 3, 3)):
        with pytest.raises(ValueError):
            ops.pack_dw3x3_weights(bad)
    with pytest.raises(ValueError):
        zoo._OwnDepthwise(zoo._ConvBNReLU6(C, C, 1))
    # the tables stay fp32 under a bf16 cast, bit for bit, while the convolution weight is cast
    cast = own.to(torch.bfloat16)
    assert cast.w9c.dtype == cast.bias.dtype == torch.float32 and torch.equal(cast.w9c, w9c)
    assert cast[0].weight.dtype == torch.bfloat16
    assert sorted(cast.state_dict()) == sorted(block.state_dict())                  # the tables are not checkpoint entries


CASES = [(2, 14, 14, 96, 1), (2, 15, 13, 96, 2), (2, 7, 7, 16, 1), (1, 7, 7, 16, 2), (2, 1, 5, 8, 1), (2, 1, 5, 8, 2),
         (2, 5, 1, 8, 1), (2, 5, 1, 8, 2), (1, 1, 1, 8, 2), (1, 2, 2, 8, 2), (3, 6, 9, 24, 2), (1, 112, 112, 8, 2)]


@pytest.mark.parametrize("b,h,w,c,s", CASES)
@pytest.mark.parametrize("relu6", [0, 1])
def test_restatement_equals_torch_grouped_convolution(b, h, w, c, s, relu6):
    """fp64: dw_fwd / dw_bwd against F.conv2d(groups=C) + bias + hardtanh(0, 6) and its autograd input gradient, to 1e-12
    relative; strides 1 and 2, odd H / W, H = 1 or W = 1."""
    name = "restate/%s" % ((b, h, w, c, s, relu6),)
    op = dref.operands(name, "gaussian", b, h, w, c, s)
    ar = Arith()
    o = dref.dw_fwd(ar, op.x, op.w9c, op.bias, s, relu6)
    xin = op.x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    wt = op.w9c.double().t().reshape(c, 1, 3, 3)
    pre = F.conv2d(xin, wt, op.bias.double(), stride=s, padding=1, groups=c)
    yref = F.hardtanh(pre, 0.0, 6.0) if relu6 else pre
    assert yref.shape == (b, c, dref.out_size(h, s), dref.out_size(w, s))
    got = dref.expected(o)
    yr = yref.detach().permute(0, 2, 3, 1)
    assert float((got - yr).abs().max()) <= 1e-12 * max(1.0, float(yr.abs().max()))
    # the gradient's mask comes from a stored y; hand both sides the same one: the fp64 output itself
    (gref,) = torch.autograd.grad(yref, xin, op.g.double().permute(0, 3, 1, 2))
    ob = dref.dw_bwd(ar, op.g, yr if relu6 else None, op.w9c, h, w, s, relu6)
    gr = gref.permute(0, 2, 3, 1)
    assert ob.pre.shape == gr.shape
    assert float((ob.pre - gr).abs().max()) <= 1e-12 * max(1.0, float(gr.abs().max()))


MUTANT_SHAPES = [(2, 14, 14, 96, 1), (2, 15, 13, 96, 2), (2, 7, 7, 960, 1)]
MUTANTS = ["trunc", "ge_mask", "le6_mask", "flip_taps", "oh_floor", "no_bias", "drop_border"]


def _exact_leg(emu):
    """The exact leg of tests/test_gpu_depthwise.py with the kernel replaced by the emulation `emu`; returns the names of
    the comparisons that failed."""
    failed = []
    for (b, h, w, c, s) in MUTANT_SHAPES:
        for leg, relu6 in (("clamp", 1), ("rounding", 0)):
            name = "mutants/%s/%s" % ((b, h, w, c, s), leg)
            op = dref.operands(name, leg, b, h, w, c, s)
            ref = dref.dw_fwd(Arith(), op.x, op.w9c, op.bias, s, relu6)
            dref.assert_premise(name + "/fwd", ref, leg)
            if leg == "clamp":
                assert min(dref.branch_shares(ref)) >= 0.10, dref.branch_shares(ref)
            y = dref.mask_source(name, leg, dref.finish(Arith(), ref)) if relu6 else None
            refb = dref.dw_bwd(Arith(), op.g, y, op.w9c, h, w, s, relu6)
            dref.assert_premise(name + "/bwd", refb, leg)
            for what, o, got in (("fwd", ref, lambda: dref.finish(emu, dref.dw_fwd(emu, op.x, op.w9c, op.bias, s, relu6))),
                                 ("bwd", refb, lambda: dref.finish(emu, dref.dw_bwd(emu, op.g, y, op.w9c, h, w, s, relu6)))):
                try:
                    dref.compare_exact(name + "/" + what, got(), o)
                except AssertionError:
                    failed.append(name + "/" + what)
    return failed


def test_exact_leg_passes_the_emulation_and_rejects_mutants():
    assert _exact_leg(Arith(F32, chunk=1)) == []
    for m in MUTANTS:
        failed = _exact_leg(Arith(F32, chunk=1, mut=(m,)))
        print(m, "rejected by", len(failed), "comparisons, e.g.", failed[:2])
        assert failed, "mutant %s passes the exact leg" % m


def test_clamp_set_populates_every_branch():
    """The figures the clamp set was chosen by, on the reference alone."""
    for (b, h, w, c, s) in MUTANT_SHAPES:
        op = dref.operands("branches/%s" % ((b, h, w, c, s),), "clamp", b, h, w, c, s)
        ref = dref.dw_fwd(Arith(), op.x, op.w9c, op.bias, s, 1)
        shares = dref.branch_shares(ref)
        print((b, h, w, c, s), "pre <= 0 / inside / pre >= 6: %.2f %.2f %.2f, max sum |terms| %.0f" % (*shares, float(ref.S.max())))
        assert min(shares) >= 0.10


def _depthwise_blocks(model):
    from dl_attack_on_imagenet_amd import zoo
    return [m for m in model.modules() if isinstance(m, zoo._OwnDepthwise)]


def test_switch_replaces_the_17_depthwise_layers_and_nothing_else():
    from dl_attack_on_imagenet_amd import zoo
    kw = dict(num_classes=10, seed=1, dtype=torch.bfloat16, channels_last=True)
    with pytest.raises(ValueError, match="own_depthwise"):
        zoo.build_classifier("resnet18", own_depthwise=True, **kw)
    with pytest.raises(ValueError, match="own_depthwise"):
        zoo.build_classifier("mobilenet", num_classes=10, seed=1, channels_last=True, own_depthwise=True)
    with pytest.raises(ValueError, match="own_depthwise"):
        zoo.build_classifier("mobilenet", num_classes=10, seed=1, dtype=torch.bfloat16, own_depthwise=True)
    off = zoo.build_classifier("mobilenet", **kw)
    on = zoo.build_classifier("mobilenet", own_depthwise=True, **kw)
    assert _depthwise_blocks(off) == []
    blocks = _depthwise_blocks(on)
    assert [(m.channels, m.stride) for m in blocks] == dref.MOBILENET_LAYERS and len(blocks) == 17
    assert dref.MOBILENET_LAYERS == [(32, 1), (96, 2), (144, 1), (144, 2), (192, 1), (192, 1), (192, 2)] + [(384, 1)] * 4 + \
        [(576, 1), (576, 1), (576, 2)] + [(960, 1)] * 3
    for m in blocks:
        assert m.w9c.shape == (9, m.channels) and m.w9c.dtype == m.bias.dtype == torch.float32
        assert m[0].weight.dtype == torch.bfloat16
    plain = zoo.build_classifier("mobilenet", num_classes=10, seed=1)
    assert sorted(off.state_dict()) == sorted(plain.state_dict()) == sorted(on.state_dict())     # torchvision key names
    for a, b in zip(off.state_dict().values(), on.state_dict().values()):
        assert torch.equal(a, b)
    assert sum(p.numel() for p in zoo.build_classifier("mobilenet", seed=1, dtype=torch.bfloat16, channels_last=True,
                                                       own_depthwise=True)[1].parameters()) == 3504872
    # off the GPU the rewritten network runs its original modules: the same function as the switch-off network
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(0)).bfloat16()
    assert torch.equal(off(x), on(x))
    # the layer table of the reference file, from the network itself at 224 x 224
    seen = []
    probe = zoo.build_classifier("mobilenet", num_classes=10, seed=1)
    for m in probe.modules():
        if zoo._is_depthwise3x3(m):
            m.register_forward_hook(lambda mod, args, out: seen.append((mod[0].out_channels, args[0].shape[2], mod[0].stride[0])))
    probe(torch.zeros(1, 3, 224, 224))
    assert seen == dref.MOBILENET_SHAPES_ALL17
    assert sorted(set(seen)) == sorted(dref.MOBILENET_SHAPES)


def test_cli_flag_defaults_to_the_library():
    import demo_dL_attack
    p = demo_dL_attack.build_parser()
    assert p.parse_args([]).own_depthwise == 0
    assert p.parse_args(["--own-depthwise", "1"]).own_depthwise == 1
    with pytest.raises(SystemExit):
        p.parse_args(["--own-depthwise", "2"])
    from test_cabi_host import test_cli_flags_match_reference
    test_cli_flags_match_reference()
