"""CPU: host side of the whole-head attention kernels (adil_attn_fwd / adil_attn_bwd): the built library exports the symbols
at ABI 8 and refuses bad arguments before any launch, the restatement of tests/attention_reference.py against torch's
softmax attention and autograd, every premise of the exact legs for every row of the GPU table, the fp32 emulation on every
leg, the comparators' power to reject mutants, and the `own_attention` switch with its fallback route, state dict and CLI
default."""
import ctypes
import os
import re

import pytest
import torch

import attention_reference as aref
from classifier_reference import Arith

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"adil_attn_max_tokens": 1, "adil_attn_fwd": 7, "adil_attn_bwd": 9}


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
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == (0 if name == "adil_attn_max_tokens" else nargs)
    bound = _lib.load()
    assert bound.adil_abi_version() == _lib.ABI_VERSION == 8
    tmax = bound.adil_attn_max_tokens()
    assert tmax >= 197 and tmax == aref.MAX_TOKENS == aref.ROWS[-1][1]
    # refusals need no device: they return before any HIP call
    f, b = bound.adil_attn_fwd, bound.adil_attn_bwd
    assert f(None, None, None, 1, 1, 1, None) == -1
    assert b(None, None, None, None, None, 1, 1, 1, None) == -1
    for (B, T, H) in [(1, 0, 1), (1, tmax + 1, 1), (1, 1, 0), (0, 1, 1), (-1, 5, 2), (2, -5, 2), (65536, 5, 65536)]:
        assert f(16, 16, 16, B, T, H, None) == -1
        assert b(16, 16, 16, 16, 16, B, T, H, None) == -1
    for i in range(3):                                                   # a NULL or misaligned pointer, each position
        for bad in (None, 24):
            args = [16, 16, 16]
            args[i] = bad
            assert f(*args, 1, 5, 2, None) == -1
    for i in range(5):
        for bad in (None, 24):
            args = [16, 16, 16, 16, 16]
            args[i] = bad
            assert b(*args, 1, 5, 2, None) == -1


@pytest.mark.parametrize("B,T,H", [(2, 5, 2), (1, 33, 3)])
def test_restatement_equals_torch(B, T, H):
    """The fp64 restatement against torch's softmax attention and autograd in fp64 on the layouts of the two linear layers, to
    1e-12; the gradient from the restatement's own o and lse and from `stored` ones alike."""
    op = aref.operands("torch", "gaussian", B, T, H)
    qkv = op.qkv.double().requires_grad_(True)
    x = qkv.reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    w = torch.softmax((x[0] @ x[1].transpose(-1, -2)) * 64 ** -0.5, dim=-1)
    o = (w @ x[2]).permute(0, 2, 1, 3).reshape(B, T, H * 64)
    g, = torch.autograd.grad(o, qkv, op.go.double())
    got = aref.attention(Arith(), op.qkv, op.go, H)
    lse = torch.logsumexp((x[0] @ x[1].transpose(-1, -2)) * 0.125, dim=-1)
    assert float((got.o - o).abs().max()) < 1e-12 and float((got.lse - lse).abs().max()) < 1e-12
    assert float((got.gqkv - g).abs().max()) < 1e-11
    again = aref.attention(Arith(), op.qkv, op.go, H, stored=(got.o, got.lse))
    assert float((again.gqkv - g).abs().max()) < 1e-11


@pytest.mark.parametrize("leg", aref.LEGS)
@pytest.mark.parametrize("row", aref.ROWS, ids=str)
def test_emulation_passes_every_row_of_the_gpu_table(row, leg):
    """The fp32 emulation passes the exact legs bit for bit and the gaussian legs under their bounds, from its own o and lse
    as the GPU tests take them; the premises (gap, 2^24, bf16 values, pi not injective) are asserted on the reference alone
    inside `exact_references`."""
    name, op, want = aref.case(row, leg)
    aref.check(name, leg, op, aref.emulate(op), want)


def test_table_holds_the_rows_the_kernels_can_go_wrong_at():
    ts = [t for _, t, _ in aref.ROWS]
    assert 1 in ts and 32 in ts and 33 in ts and 197 in ts and aref.MAX_TOKENS in ts
    assert any(t % 32 for t in ts) and any(h > 1 for _, _, h in aref.ROWS) and any(b > 1 for b, _, _ in aref.ROWS)
    assert (2, 197, 12) in aref.ROWS


MUTANT_ROWS = [(2, 5, 2), (1, 33, 2)]


@pytest.mark.parametrize("mut", aref.MUTANTS)
def test_comparators_reject_the_mutants(mut):
    """A kernel without the scale or with it twice, with padded keys unmasked, with padded query rows counted in gk / gv,
    without delta, with dS transposed, with gk unscaled, with k and v swapped, reading the next head's columns, with the
    softmax over the query axis, or with lse = m fails at least one leg of a small row."""
    failed = []
    for row in MUTANT_ROWS:
        for leg in aref.LEGS:
            name, op, want = aref.case(row, leg)
            try:
                aref.check(name, leg, op, aref.emulate(op, mut=(mut,)), want)
            except AssertionError:
                failed.append((row, leg))
    print(mut, "fails", failed)
    assert failed, f"no leg rejects the mutant {mut}"


def _small_vit():
    from dl_attack_on_imagenet_amd import zoo
    torch.manual_seed(5)
    return zoo.VisionTransformer(image_size=32, layers=2, heads=2, dim=128, mlp_dim=256, num_classes=10).eval()


def test_switch_keeps_the_function_and_the_state_dict_on_the_fallback_route():
    """With the switch on, a CPU fp32 network runs exactly the statements it runs today (the kernels do not cover it): equal
    logits, bit for bit; state-dict keys and values are unchanged and load_state_dict round-trips."""
    from dl_attack_on_imagenet_amd import zoo
    net = _small_vit()
    keys = list(net.state_dict().keys())
    x = torch.randn(3, 3, 32, 32)
    with torch.no_grad():
        want = net(x)
    assert all(not m.own_attention for m in net.modules() if isinstance(m, zoo._EncoderBlock))
    assert zoo.use_own_attention_(net) == 2
    assert all(m.own_attention for m in net.modules() if isinstance(m, zoo._EncoderBlock))
    with torch.no_grad():
        got = net(x)
    assert torch.equal(got, want)
    assert list(net.state_dict().keys()) == keys
    other = _small_vit()
    other.load_state_dict(net.state_dict())
    zoo.use_own_attention_(other)
    net.load_state_dict(other.state_dict())
    with torch.no_grad():
        assert torch.equal(other(x), want)
    with pytest.raises(ValueError):
        zoo.use_own_attention_(torch.nn.Sequential(torch.nn.Linear(4, 4)))


def test_vit_b_16_has_12_blocks_and_the_kernels_cover_its_sequence():
    from dl_attack_on_imagenet_amd import ops, zoo
    with torch.device("meta"):
        net = zoo.VisionTransformer()
    assert zoo.use_own_attention_(net) == 12
    assert (224 // 16) ** 2 + 1 == 197 <= aref.MAX_TOKENS and 768 // 12 == ops.ATTN_HEAD_DIM
    assert not ops.attention_covers(torch.zeros(2, 197, 3 * 768, dtype=torch.bfloat16), 12)      # CPU: not covered
    with pytest.raises(ValueError):
        ops.attention(torch.zeros(2, 197, 3 * 768, dtype=torch.bfloat16), 12)                    # and no CPU fallback in ops


def test_build_classifier_switch():
    """own_attention is valid only for vit_b_16 in bf16; it needs no channels_last; the default is off."""
    from dl_attack_on_imagenet_amd import zoo
    for name in ("resnet18", "mobilenet_v2", "densenet121"):
        with pytest.raises(ValueError, match="own_attention is a switch of ViT-B/16"):
            zoo.build_classifier(name, num_classes=10, dtype=torch.bfloat16, own_attention=True)
    with pytest.raises(ValueError, match="own_attention needs a bfloat16 network"):
        zoo.build_classifier("vit_b_16", num_classes=10, dtype=torch.float32, own_attention=True)
    import inspect
    assert inspect.signature(zoo.build_classifier).parameters["own_attention"].default is False


def test_cli_switch_defaults_to_off():
    import demo_dL_attack
    p = demo_dL_attack.build_parser()
    assert p.parse_args([]).own_attention == 0
    assert p.parse_args(["--own-attention", "1"]).own_attention == 1
