"""GPU: the whole-head attention kernels (adil_attn_fwd / adil_attn_bwd, csrc/adil_attention.hip) through the C ABI against
the fp64 restatement of tests/attention_reference.py — bit for bit on the two selection legs, under the derived elementwise
bounds on the two gaussian legs — their contract (extents, every element written, refusals, reproducibility), the autograd
function, and the ViT that runs its attention on them (`own_attention`)."""
import os
import subprocess
import sys

import pytest
import torch

import attention_reference as aref
from classifier_reference import BF16, CANARY, F32
from graph_tools import assert_graph_used, no_capture_fallback

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PAD = 256                        # canary elements in front of and behind every output


def ops():
    from dl_attack_on_imagenet_amd import ops as o
    return o


def _lib():
    return __import__("dl_attack_on_imagenet_amd._lib", fromlist=["x"]).load()


def _bf16_depth_bound(layers: int) -> float:
    """The bound of tests/test_gpu_stem.py, restated: mean |logit error| of a bf16-activation network against its fp32
    twin relative to the rms logit; `layers` roundings of relative size 2^-9 in series add in quadrature, times 2 for a
    relative gain above 1 in a random-weight network."""
    return 2.0 * 2.0 ** -9 * layers ** 0.5


def _vit_roundings(blocks: int) -> int:
    """bf16 roundings in series through a ViT: per block LayerNorm, in-projection, attention, out-projection + residual,
    LayerNorm, fc1, GELU, fc2 + residual; the patch embedding, the final LayerNorm and the head."""
    return 8 * blocks + 3


def _dev(t):
    return t.to(DEV).contiguous()


def _guarded(shape, dtype):
    """An output of `shape` inside a canary-filled buffer (the output itself holds CANARY too); returns (buffer, view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), CANARY, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n].view(shape)


def _intact(buf):
    return bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all())


def _run_fwd(qkv, H):
    o, lib = ops(), _lib()
    B, T, _ = qkv.shape
    obuf, out = _guarded((B, T, H * 64), BF16)
    lbuf, lse = _guarded((B, H, T), F32)
    assert lib.adil_attn_fwd(o._ptr(qkv), o._ptr(out), o._ptr(lse), B, T, H, o._stream()) == 0
    torch.cuda.synchronize()
    assert _intact(obuf) and _intact(lbuf), "forward wrote outside o / lse"
    assert not bool((out == CANARY).any()) and not bool((lse == CANARY).any()), "forward left elements of o / lse unwritten"
    return out, lse


def _run_bwd(qkv, out, lse, go, H):
    o, lib = ops(), _lib()
    B, T, _ = qkv.shape
    gbuf, gqkv = _guarded((B, T, 3 * H * 64), BF16)
    assert lib.adil_attn_bwd(o._ptr(qkv), o._ptr(out), o._ptr(lse), o._ptr(go), o._ptr(gqkv), B, T, H, o._stream()) == 0
    torch.cuda.synchronize()
    assert _intact(gbuf), "gradient wrote outside gqkv"
    assert not bool((gqkv == CANARY).any()), "gradient left elements of gqkv unwritten"
    return gqkv


def _run(op, wrap=_dev):
    """Both kernels on one operand set -> attention_reference.Results of device tensors."""
    qkv = wrap(op.qkv)
    out, lse = _run_fwd(qkv, op.H)
    return aref.Results(out, lse, _run_bwd(qkv, wrap(out), lse, wrap(op.go), op.H))


def _same_bits(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("leg", aref.LEGS)
@pytest.mark.parametrize("row", aref.ROWS, ids=str)
def test_attention_against_the_fp64_restatement(row, leg):
    """Every row on every leg through the C ABI, forward and gradient: o and gqkv bit for bit on the selection legs (lse
    under its bound), max |err| / bound <= 1 for o, lse and gqkv on the gaussian legs (gqkv restated from the stored o and
    lse); canaries around the outputs intact, none left inside; the same call twice gives equal bits."""
    name, op, want = aref.case(row, leg)
    got = _run(op)
    aref.check(name, leg, op, aref.Results(*(t.cpu() for t in got)), want)
    again = _run(op)
    for a, b in zip(got, again):
        assert _same_bits(a, b), name


def _in_nan(t):
    """t as a slice of a larger buffer whose surroundings hold NaN bit patterns (one row in front, one behind)."""
    t = t.to(DEV)
    big = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=DEV)
    big[1:-1] = t
    view = big[1:-1]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


@pytest.mark.parametrize("row", [(2, 5, 2), (1, 33, 2), (2, 197, 12)], ids=str)
def test_attention_reads_nothing_outside_its_operands(row):
    """qkv, o and go as slices of larger buffers whose surroundings are NaN: bitwise the results of the plain call."""
    name, op, _ = aref.case(row, "gaussian")
    plain, fenced = _run(op), _run(op, wrap=_in_nan)
    for a, b in zip(plain, fenced):
        assert bool(torch.isfinite(b.float()).all()) and _same_bits(a, b), name


def test_attention_refuses_and_leaves_outputs_untouched():
    o, lib = ops(), _lib()
    tmax = lib.adil_attn_max_tokens()
    assert tmax == aref.MAX_TOKENS >= 197
    B, T, H = 2, 5, 2
    op = aref.operands("refuse", "gaussian", B, tmax + 1, H)
    qkv, go = _dev(op.qkv), _dev(op.go)
    obuf, out = _guarded((B, tmax + 1, H * 64), BF16)
    lbuf, lse = _guarded((B, H, tmax + 1), F32)
    gbuf, gqkv = _guarded((B, tmax + 1, 3 * H * 64), BF16)
    st = o._stream()
    p = o._ptr
    for (b, t, h) in [(B, 0, H), (B, tmax + 1, H), (B, T, 0), (0, T, H), (B, -1, H)]:
        assert lib.adil_attn_fwd(p(qkv), p(out), p(lse), b, t, h, st) == EINVAL
        assert lib.adil_attn_bwd(p(qkv), p(out), p(lse), p(go), p(gqkv), b, t, h, st) == EINVAL
    for i in range(3):
        args = [p(qkv), p(out), p(lse)]
        args[i] = None
        assert lib.adil_attn_fwd(*args, B, T, H, st) == EINVAL
    for i in range(5):
        args = [p(qkv), p(out), p(lse), p(go), p(gqkv)]
        args[i] = None
        assert lib.adil_attn_bwd(*args, B, T, H, st) == EINVAL
    assert lib.adil_attn_fwd(qkv.data_ptr() + 8, p(out), p(lse), B, T, H, st) == EINVAL       # misaligned
    torch.cuda.synchronize()
    for buf in (obuf, lbuf, gbuf):
        assert bool((buf == CANARY).all()), "a refused call wrote to its outputs"
    x = torch.zeros(2, 5, 3 * 128, dtype=BF16, device=DEV)
    assert o.attention_covers(x, 2) and not o.attention_covers(x, 3) and not o.attention_covers(x.float(), 2)
    assert not o.attention_covers(x[:, :, :192], 1) and not o.attention_covers(x.cpu(), 2)
    assert not o.attention_covers(torch.zeros(1, tmax + 1, 192, dtype=BF16, device=DEV), 1)
    with pytest.raises(ValueError):
        o.attention(x.float(), 2)


@pytest.mark.parametrize("row", [(2, 17, 3), (2, 197, 12)], ids=str)
def test_autograd_function_equals_the_c_abi_bitwise(row):
    """ops.attention under autograd, with a contiguous and with a strided output gradient, equals the C-ABI results."""
    o = ops()
    B, T, H = row
    op = aref.operands("autograd/%s" % (row,), "gaussian", B, T, H)
    want = _run(op)
    qkv = _dev(op.qkv).requires_grad_(True)
    out = o.attention(qkv, H)
    assert out.shape == (B, T, H * 64) and out.dtype == BF16 and out.is_contiguous()
    (g,) = torch.autograd.grad(out, qkv, _dev(op.go), retain_graph=True)
    assert _same_bits(out, want.o) and _same_bits(g, want.gqkv)
    wide = torch.zeros(B, T, 2 * H * 64, dtype=BF16, device=DEV)
    wide[:, :, :H * 64] = _dev(op.go)
    strided = wide[:, :, :H * 64]
    assert not strided.is_contiguous()
    (g2,) = torch.autograd.grad(out, qkv, strided)
    assert _same_bits(g2, want.gqkv)


def test_attention_is_bitwise_across_processes():
    """Two fresh child processes, one after the other (the second only if the first exited 0), each under `timeout`:
    byte-identical o and gqkv for three shapes."""
    child = os.path.join(ROOT, "tests", "attention_child.py")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
    outs = []
    for _ in range(2):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, child], env=env, capture_output=True, text=True,
                           timeout=270, cwd=ROOT)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("hash ")]
        assert len(lines) == 6, r.stdout[-2000:]
        outs.append(lines)
    for a, b in zip(*outs):
        assert a == b, (a, b)


# ------------------------------------------------------------------------------------------------------------- network
def _small_vit(dtype, own):
    from dl_attack_on_imagenet_amd import zoo
    torch.manual_seed(5)
    vit = zoo.VisionTransformer(image_size=32, layers=2, heads=2, dim=128, mlp_dim=256, num_classes=10)
    with torch.no_grad():                                               # a class token and attention that are not trivial
        vit.class_token.normal_(std=0.5)
        vit.encoder.pos_embedding.normal_(std=0.5)
    if own:
        assert zoo.use_own_attention_(vit) == 2
    net = torch.nn.Sequential(zoo.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225]), vit).eval()
    for q in net.parameters():
        q.requires_grad_(False)
    return net.to(device=DEV, dtype=dtype)


def _forward_and_gradient(model, x):
    x = x.clone().requires_grad_(True)
    out = model(x)
    logits = out.float()
    (g,) = torch.autograd.grad(logits.square().sum(), x)
    assert g.shape == x.shape and g.dtype == x.dtype
    return out.dtype, logits.detach(), g.detach().float()


def _op_counts(model, x):
    """aten calls of forward + input gradient whose name holds `softmax` resp. is a batched matmul."""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.softmax = self.bmm = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = func.overloadpacket.__name__
            self.softmax += "softmax" in name
            self.bmm += name in ("bmm", "baddbmm")
            return func(*args, **(kwargs or {}))

    with Count() as c:
        _forward_and_gradient(model, x)
    return c.softmax, c.bmm


def _compare_with_fp32_twin(tag, ref, plain, own, x, blocks):
    _, lr, gr = _forward_and_gradient(ref, x.float())
    _, l0, g0 = _forward_and_gradient(plain, x)
    d1, l1, g1 = _forward_and_gradient(own, x)
    rms = float(lr.square().mean().sqrt())
    n = _vit_roundings(blocks)
    bound_l = _bf16_depth_bound(n) * rms
    # the gradient passes the same layers again (2 n roundings in series) and starts from 2 * logits, which carry the
    # logits' own relative error
    bound_g = _bf16_depth_bound(2 * n) + _bf16_depth_bound(n)
    rel = lambda g: float((g - gr).norm() / gr.norm())
    e0, e1, r0, r1 = float((l0 - lr).abs().mean()), float((l1 - lr).abs().mean()), rel(g0), rel(g1)
    print("%s: logit error vs fp32: switch off %.5f on %.5f, rms %.4f, bound %.5f; input gradient relative error vs fp32: "
          "switch off %.4f on %.4f, bound %.4f" % (tag, e0, e1, rms, bound_l, r0, r1, bound_g))
    assert d1 == BF16 and bool(torch.isfinite(l1).all()) and bool(torch.isfinite(g1).all()) and float(gr.abs().max()) > 0
    assert float(g1.abs().max()) > 0
    assert e1 <= bound_l, (e0, e1, rms)
    assert r1 <= bound_g, (r0, r1)


def test_small_vit_on_the_attention_kernels():
    """The 2-layer ViT of the CPU tests in bf16 with the switch on: no softmax and no batched matmul is left in forward +
    input gradient (2 softmax calls — forward and backward — and at least 4 batched matmuls per layer with it off: 6 where
    autograd forms both operand gradients of both products with one call each); logits
    and input gradient within the bf16 depth bound of the fp32 twin, the switch-off network's error printed next to it."""
    x = torch.rand(6, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(DEV).to(BF16)
    ref, plain, own = _small_vit(F32, False), _small_vit(BF16, False), _small_vit(BF16, True)
    s0, m0 = _op_counts(plain, x)
    s1, m1 = _op_counts(own, x)
    print("softmax / batched-matmul calls in forward + input gradient: switch off %d / %d, on %d / %d" % (s0, m0, s1, m1))
    assert (s1, m1) == (0, 0) and s0 == 2 * 2 and m0 >= 4 * 2
    _compare_with_fp32_twin("small ViT", ref, plain, own, x, 2)


def test_vit_b_16_on_the_attention_kernels():
    """build_classifier("vit_b_16", dtype=bf16, own_attention=True) at 2 images of 224 x 224: 12 blocks switched, finite
    logits and input gradient, under the same bound against the fp32 twin."""
    from dl_attack_on_imagenet_amd import zoo
    kw = dict(num_classes=100, seed=3, device=DEV)
    ref = zoo.build_classifier("vit_b_16", **kw)
    plain = zoo.build_classifier("vit_b_16", dtype=BF16, **kw)
    own = zoo.build_classifier("vit_b_16", dtype=BF16, own_attention=True, **kw)
    blocks = [m for m in own.modules() if isinstance(m, zoo._EncoderBlock)]
    assert len(blocks) == 12 and all(m.own_attention for m in blocks)
    assert not any(m.own_attention for m in plain.modules() if isinstance(m, zoo._EncoderBlock))
    x = torch.rand(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)).to(DEV).to(BF16)
    s1, m1 = _op_counts(own, x)
    assert (s1, m1) == (0, 0)
    _compare_with_fp32_twin("ViT-B/16", ref, plain, own, x, 12)


def test_attention_in_a_graphed_solver():
    """The small ViT with the switch on under engine.DDragueSolver(...).run(n, use_graph=True) returns the eager loop's
    adversarial images bit for bit: the kernels launch on the capturing stream and neither synchronise nor allocate outside
    the allocator."""
    from dl_attack_on_imagenet_amd import engine
    o = ops()
    net = _small_vit(BF16, True)
    g = torch.Generator().manual_seed(12)
    x = torch.rand(8, 3, 32, 32, generator=g).to(DEV).to(BF16)
    d = (-1 + 2 * torch.rand(3, 32, 32, 6, generator=g)).to(DEV)
    eager = engine.DDragueSolver(net, x, d, 0.1, "logits").run(9)
    with no_capture_fallback():                                     # a failed capture is an error, not an eager run
        graphed = engine.DDragueSolver(net, x, d, 0.1, "logits").run(9, use_graph=True)
    assert_graph_used(graphed)
    adv_e, adv_g = eager.result()[0], graphed.result()[0]
    assert graphed.iters == 9 and bool(torch.isfinite(adv_e.float()).all()) and bool((adv_e != x).any())
    assert _same_bits(adv_e, adv_g)
    assert o.attention_covers(torch.zeros(8, 5, 3 * 128, dtype=BF16, device=DEV), 2)
