"""CPU: host side of the stride-2 3x3 convolution (adil_conv3x3_s2_fwd / _bwd): the built library exports the symbols and
the header declares them, the gradient weight packing against an fp64 restatement of the parity-class formula, the
switch's argument checks and the CLI default."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adil_conv3x3_s2_fwd", "adil_conv3x3_s2_bwd")


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
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 9
    bound = _lib.load()
    assert bound.adil_abi_version() == _lib.ABI_VERSION == 8
    assert bound.adil_max_atoms() == 128
    from dl_attack_on_imagenet_amd import ops
    assert int(re.search(r"#define\s+ADIL_CONV3X3_S2_MAX_W\s+(\d+)", src).group(1)) == ops.CONV3X3_S2_MAX_W


def _parity_class_gradient(g, wpb, h, w):
    """gx[b][2i+ph][2j+pw][c] = sum over kh in KH(ph), kw in KW(pw), n of g[b][i + [kh = 0]][j + [kw = 0]][n] *
    wpb[c][kh*3+kw][n], KH(0) = {1}, KH(1) = {0, 2} (same for kw), sources outside the OH x OW grid dropped — what
    adil_conv3x3_s2_bwd computes, in fp64 on (B, OH, OW, N) / (C, 9, N) tensors."""
    b, oh, ow, n = g.shape
    c = wpb.shape[0]
    gx = torch.zeros(b, h, w, c, dtype=torch.float64)
    taps = {0: (1,), 1: (0, 2)}
    for ph in (0, 1):
        for pw in (0, 1):
            acc = torch.zeros(b, oh, ow, c, dtype=torch.float64)
            for kh in taps[ph]:
                for kw in taps[pw]:
                    dh, dw = int(kh == 0), int(kw == 0)
                    src = torch.zeros_like(g)
                    src[:, :oh - dh, :ow - dw] = g[:, dh:, dw:]
                    acc += src @ wpb[:, kh * 3 + kw, :].t()
            gx[:, ph::2, pw::2] = acc
    return gx


@pytest.mark.parametrize("b,h,w,c,n", [(2, 8, 12, 64, 128), (1, 2, 2, 64, 64), (3, 6, 10, 128, 64), (1, 56, 56, 64, 64)])
def test_gradient_weight_packing_against_parity_class_formula(b, h, w, c, n):
    from dl_attack_on_imagenet_amd import ops
    gen = torch.Generator().manual_seed(b + h + w + c + n)
    wt = (torch.randn(n, c, 3, 3, generator=gen) / (9 * c) ** 0.5).bfloat16()
    wf, wb = ops.pack_conv3x3_s2_weights(wt)
    assert wf.shape == (n, 9 * c) and wb.shape == (c, 9 * n) and wf.dtype == wb.dtype == torch.bfloat16
    w64 = wt.double()
    assert torch.equal(wf.double().reshape(n, 3, 3, c), w64.permute(0, 2, 3, 1))           # [n][kh*3+kw][c]
    assert torch.equal(wf, ops.pack_conv3x3_weights(wt)[0])                                 # the layout of adil_conv3x3
    assert torch.equal(wb.double().reshape(c, 3, 3, n), w64.permute(1, 2, 3, 0))           # [c][kh*3+kw][n], not flipped
    g = torch.randn(b, h // 2, w // 2, n, generator=gen, dtype=torch.float64)
    x = torch.zeros(b, c, h, w, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w64, stride=2, padding=1).backward(g.permute(0, 3, 1, 2))
    ref = x.grad.permute(0, 2, 3, 1)
    got = _parity_class_gradient(g, wb.double().reshape(c, 9, n), h, w)
    assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    with pytest.raises(ValueError):
        ops.pack_conv3x3_s2_weights(torch.zeros(64, 64, 1, 1))


def test_switch_needs_the_fused_path_and_marks_the_layers():
    from dl_attack_on_imagenet_amd import zoo
    with pytest.raises(ValueError, match="own_strided_conv"):
        zoo.build_classifier("resnet18", num_classes=10, own_strided_conv=True)
    off = zoo.build_classifier("resnet50", num_classes=10, seed=1, fuse_bn_act=True)[1]
    on = zoo.build_classifier("resnet50", num_classes=10, seed=1, fuse_bn_act=True, own_strided_conv=True)[1]
    assert off.own_strided_conv is False and on.own_strided_conv is True
    marked = [i for i, blk in enumerate(on.layers) if blk.c2.own_strided_conv]
    assert marked == [3, 7, 13]                                   # first bottleneck of stages 2-4: the three layers
    assert not any(m.own_strided_conv for blk in off.layers for m in blk.children() if isinstance(m, zoo._ConvAffine))
    assert not any(k.startswith(("wp_s2",)) or ".wp_s2" in k for k in off.state_dict())
    c2 = on.layers[3].c2
    assert c2.wp_s2_fwd.shape == (128, 9 * 128) and c2.wp_s2_bwd.shape == (128, 9 * 128)
    r18 = zoo.build_classifier("resnet18", num_classes=10, seed=1, fuse_bn_act=True, own_strided_conv=True)[1]
    assert [i for i, blk in enumerate(r18.layers) if blk.c1.own_strided_conv] == [2, 4, 6]
    assert r18.layers[2].c1.wp_s2_bwd.shape == (64, 9 * 128)


def test_cli_flag_defaults_to_the_library():
    import demo_dL_attack
    p = demo_dL_attack.build_parser()
    assert p.parse_args([]).own_strided_conv == 0
    assert p.parse_args(["--own-strided-conv", "1"]).own_strided_conv == 1
    with pytest.raises(SystemExit):
        p.parse_args(["--own-strided-conv", "2"])
    from test_cabi_host import test_cli_flags_match_reference
    test_cli_flags_match_reference()
