"""GPU: the strided dense kernels (adil_dense1x1_fwd_ld / _bwd_ld, adil_dense3x3_fwd_ld / _bwd_ld) through the C ABI —
bit for bit against the plain entry points on the same values embedded in wider buffers, `accumulate = 1` against the fp64
restatement of tests/dense_block_reference.py — and the dense-block path built on them: `ops.dense_block` /
`zoo._OwnDenseBlock` against the two-switch block, and the DenseNet-121 with `own_dense_block=True`."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

import dense1x1_reference as d1
import dense3x3_reference as d3
import dense_block_reference as db
from classifier_reference import BF16, CANARY

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAD = 5                          # canary rows behind every output
NAN = float("nan")


def ops():
    from dl_attack_on_imagenet_amd import ops as o
    return o


def _lib():
    return __import__("dl_attack_on_imagenet_amd._lib", fromlist=["x"]).load()


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _bf16_depth_bound(layers: int) -> float:
    """The bound of tests/test_gpu_stem.py, restated: mean |logit error| of a bf16-activation network against its fp32
    twin relative to the rms logit; `layers` roundings of relative size 2^-9 in series add in quadrature, times 2 for a
    relative gain above 1 in a random-weight network."""
    return 2.0 * 2.0 ** -9 * layers ** 0.5


class Strided:
    """A [rows][width] bf16 operand as columns [off, off + width) of a [rows + pad][ld] buffer filled with `fill`."""

    def __init__(self, t, ld, off=0, fill=NAN, pad=0, rows=None, width=None):
        rows = t.shape[0] if rows is None else rows
        self.width = t.shape[1] if width is None else width
        self.rows, self.off, self.ld, self.fill = rows, off, ld, fill
        self.buf = torch.full((rows + pad, ld), fill, dtype=BF16, device=DEV)
        if t is not None:
            self.buf[:rows, off:off + self.width] = t.to(DEV).reshape(rows, self.width)
        self.ptr = ops()._ptr(self.buf[:, off:])
        assert self.buf[:, off:].data_ptr() % 16 == 0

    def value(self):
        return self.buf[:self.rows, self.off:self.off + self.width]

    def outside_intact(self):
        """Every element that is not the operand still holds the fill value."""
        m = torch.ones_like(self.buf, dtype=torch.bool)
        m[:self.rows, self.off:self.off + self.width] = False
        rest = self.buf[m]
        return bool(torch.isnan(rest).all()) if self.fill != self.fill else bool((rest == self.fill).all())


def _out(rows, width, ld, off=0):
    return Strided(None, ld, off, CANARY, PAD, rows, width)


# ------------------------------------------------------------------------------------------------------ 1x1, strided
def _d1_plain(r, act, M, K, N):
    """(y, gx) of the plain entry points on contiguous operands."""
    o, lib, q = ops(), _lib(), r.ops
    P, S = o._ptr, o._stream
    x, w, wt, g = _dev(q.x), _dev(q.w), _dev(q.wt), _dev(q.g)
    ps, pb, sc, sh = _dev(q.pscale), _dev(q.pshift), _dev(q.scale), _dev(q.shift)
    yin = _dev(r.y)
    y = torch.full((M + PAD, N), CANARY, dtype=BF16, device=DEV)
    gx = torch.full((M + PAD, K), CANARY, dtype=BF16, device=DEV)
    assert lib.adil_dense1x1_fwd(P(x), P(ps), P(pb), P(w), P(sc), P(sh), P(y), M, K, N, act, S()) == 0
    assert lib.adil_dense1x1_bwd(P(g), P(yin), P(sc), P(wt), P(x), P(ps), P(pb), P(gx), M, K, N, act, S()) == 0
    torch.cuda.synchronize()
    assert bool((y[M:] == CANARY).all()) and bool((gx[M:] == CANARY).all())
    return y[:M], gx[:M]


def _d1_bwd_ld(r, act, M, K, N, ld, accumulate, old=None):
    """adil_dense1x1_bwd_ld with every operand strided: g, y at pitch N + 8, xin, gx at pitch ld; inputs in NaN, gx in
    canaries (its prefix preloaded with `old`).  Returns the gx Strided."""
    o, lib, q = ops(), _lib(), r.ops
    P, S = o._ptr, o._stream
    g, xin = Strided(q.g, N + 8), Strided(q.x, ld)
    yin = Strided(r.y, N + 8) if act else None
    gx = _out(M, K, ld)
    if old is not None:
        gx.buf[:M, :K] = old.to(DEV)
    sc, wt, ps, pb = _dev(q.scale), _dev(q.wt), _dev(q.pscale), _dev(q.pshift)       # held until the synchronise
    rc = lib.adil_dense1x1_bwd_ld(g.ptr, N + 8, yin.ptr if act else None, N + 8, P(sc), P(wt), xin.ptr, ld, P(ps), P(pb), gx.ptr,
                                  ld, accumulate, M, K, N, act, S())
    assert rc == 0
    torch.cuda.synchronize()
    return gx


@pytest.mark.parametrize("row", db.D1_LD_ROWS, ids=str)
def test_dense1x1_strided_equals_dense_bitwise(row):
    """Both directions (accumulate = 0) on both legs: the _ld entry on operands embedded in wider buffers gives the bits
    of the plain entry on contiguous ones.  Unused input columns hold NaN (a read outside the width shows), unused output
    columns and PAD rows behind hold canaries and stay intact."""
    M, K, N, act, ld = row
    o, lib = ops(), _lib()
    P, S = o._ptr, o._stream
    for leg in (db.exact_leg(act), "gaussian"):
        r, _, _ = db.reference_row(row, leg)
        q = r.ops
        want_y, want_gx = _d1_plain(r, act, M, K, N)
        x, y = Strided(q.x, ld), _out(M, N, N + 8)
        ps, pb, w, sc, sh = _dev(q.pscale), _dev(q.pshift), _dev(q.w), _dev(q.scale), _dev(q.shift)    # held until the synchronise
        rc = lib.adil_dense1x1_fwd_ld(x.ptr, ld, P(ps), P(pb), P(w), P(sc), P(sh), y.ptr, N + 8, M, K, N, act, S())
        assert rc == 0
        torch.cuda.synchronize()
        assert not bool(torch.isnan(y.value()).any()) and _same(y.value(), want_y), (row, leg)
        assert y.outside_intact(), (row, leg)
        gx = _d1_bwd_ld(r, act, M, K, N, ld, 0)
        assert not bool(torch.isnan(gx.value()).any()) and _same(gx.value(), want_gx), (row, leg)
        assert gx.outside_intact(), (row, leg)


@pytest.mark.parametrize("row", db.D1_LD_ROWS, ids=str)
def test_dense1x1_accumulate_against_the_fp64_restatement(row):
    """accumulate = 1 into the K-wide prefix of a wider gradient buffer preloaded with `old`: the exact leg bit for bit
    against the restatement (one fp32 add, ONE rounding; -0.0 under a masked element becomes +0), the gaussian leg under
    its bound (ratio printed); a second call on a fresh copy identical in bits; everything behind the prefix unchanged.
    Rows, operands and premises are those of tests/test_dense_block_cpu.py.
    Recorded on an MI355X, gaussian max |err| / bound in row order: 0.562, 0.930, 0.964, 0.968, 0.983, 0.955."""
    M, K, N, act, ld = row
    name = db.row_name(*row)
    r, old, acc = db.reference_row(row, db.exact_leg(act))
    gx = _d1_bwd_ld(r, act, M, K, N, ld, 1, old)
    d1.compare_exact(name + "/acc/exact", gx.value().cpu(), acc)
    assert gx.outside_intact(), name
    r, old, acc = db.reference_row(row, "gaussian")
    gx = _d1_bwd_ld(r, act, M, K, N, ld, 1, old)
    ratio = d1.gaussian_ratio(gx.value().cpu(), acc)
    print(name, "accumulate, gaussian max |err| / bound: %.3f" % ratio)
    assert ratio <= 1.0, (name, ratio)
    assert gx.outside_intact(), name
    again = _d1_bwd_ld(r, act, M, K, N, ld, 1, old)
    assert _same(again.buf, gx.buf)


# ------------------------------------------------------------------------------------------------------ 3x3, strided
def _side(t, width, rows, out):
    """The 32-wide side lives at channel offset D3_OFF of a D3_LD-wide buffer; any other width gets the pitch width + 8."""
    ld, off = (db.D3_LD, db.D3_OFF) if width == 32 else (width + 8, 0)
    return _out(rows, width, ld, off) if out else Strided(t.reshape(rows, width), ld, off)


def _d3_ld(entry, src, wp, row, R, O):
    B, H, W, C, N = row
    o, lib = ops(), _lib()
    M = B * H * W
    s, out = _side(src, R, M, False), _side(None, O, M, True)
    assert getattr(lib, entry)(s.ptr, s.ld, o._ptr(wp), out.ptr, out.ld, B, H, W, C, N, o._stream()) == 0
    torch.cuda.synchronize()
    assert out.outside_intact(), (entry, row)
    return out.value()


def _d3_plain(entry, src, wp, row, O):
    B, H, W, C, N = row
    o, lib = ops(), _lib()
    M = B * H * W
    out = torch.full((M + PAD, O), CANARY, dtype=BF16, device=DEV)
    assert getattr(lib, entry)(o._ptr(src), o._ptr(wp), o._ptr(out), B, H, W, C, N, o._stream()) == 0
    torch.cuda.synchronize()
    assert bool((out[M:] == CANARY).all())
    return out[:M]


@pytest.mark.parametrize("row", db.D3_LD_ROWS, ids=str)
def test_dense3x3_strided_equals_dense_bitwise(row):
    """Forward into (or out of) a 32-channel slice at offset 96 of a 256-wide buffer, gradient out of (or into) it, on both
    legs: the bits of the plain entry points.  NaN around every strided input, canaries around every strided output."""
    B, H, W, C, N = row
    for leg in ("exact", "gaussian"):
        r = d3.reference_row(row, leg)
        x, g, wp, wp_bwd = _dev(r.ops.x), _dev(r.ops.g), _dev(r.wp), _dev(r.wp_bwd)
        want_y, want_gx = _d3_plain("adil_dense3x3_fwd", x, wp, row, N), _d3_plain("adil_dense3x3_bwd", g, wp_bwd, row, C)
        y = _d3_ld("adil_dense3x3_fwd_ld", x, wp, row, C, N)
        gx = _d3_ld("adil_dense3x3_bwd_ld", g, wp_bwd, row, N, C)
        assert not bool(torch.isnan(y).any()) and _same(y, want_y), (row, leg)
        assert not bool(torch.isnan(gx).any()) and _same(gx, want_gx), (row, leg)


@pytest.mark.parametrize("poison", [NAN, float("inf")], ids=["nan", "inf"])
def test_selection_survives_the_stride(poison):
    """The MASK_ROW case of tests/test_gpu_dense3x3.py through the _ld entries, out of and into a slice: image 1 filled
    with NaN, and with +Inf, leaves images 0 and 2 bitwise clean and finite."""
    row = db.MASK_ROW
    B, H, W, C, N = row
    r = d3.reference_row(row, "exact")
    for entry, src, wp, R, O in (("adil_dense3x3_fwd_ld", r.ops.x, r.wp, C, N), ("adil_dense3x3_bwd_ld", r.ops.g, r.wp_bwd, N, C)):
        clean = _d3_ld(entry, _dev(src), _dev(wp), row, R, O).reshape(B, H * W, O)
        bad = _dev(src).clone()
        bad[1] = poison
        got = _d3_ld(entry, bad, _dev(wp), row, R, O).reshape(B, H * W, O)
        for img in (0, 2):
            assert bool(torch.isfinite(got[img]).all())
            assert _same(got[img], clean[img])
        assert not bool(torch.isfinite(got[1]).all())                 # the poison was really there


def test_ld_entries_refuse_and_leave_outputs_untouched():
    """A too small and a misaligned pitch and accumulate = 2 on the device: ADIL_EINVAL, canary outputs intact after a
    synchronise."""
    o, lib = ops(), _lib()
    big = torch.zeros(1 << 16, dtype=BF16, device=DEV)
    tab = torch.ones(256, dtype=torch.float32, device=DEV)
    out = torch.full((1 << 16,), CANARY, dtype=BF16, device=DEV)
    P, S = o._ptr, o._stream
    b, t, y = P(big), P(tab), P(out)
    for ldx, ldy in ((56, 32), (68, 32), (64, 24), (64, 36)):
        assert lib.adil_dense1x1_fwd_ld(b, ldx, t, t, b, t, t, y, ldy, 8, 64, 32, 1, S()) == -1
    for ldg, ldy, ldxin, ldgx, acc in ((24, 32, 64, 64, 0), (32, 36, 64, 64, 0), (32, 32, 56, 64, 1), (32, 32, 64, 68, 1),
                                       (32, 32, 64, 64, 2), (32, 32, 64, 64, -1)):
        assert lib.adil_dense1x1_bwd_ld(b, ldg, b, ldy, t, b, b, ldxin, t, t, y, ldgx, acc, 8, 64, 32, 1, S()) == -1
    for f, win, wout in ((lib.adil_dense3x3_fwd_ld, 64, 32), (lib.adil_dense3x3_bwd_ld, 32, 64)):
        for ldi, ldo in ((win - 8, wout), (win + 4, wout), (win, wout - 8), (win, wout + 4)):
            assert f(b, ldi, b, y, ldo, 2, 4, 4, 64, 32, S()) == -1
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())


# --------------------------------------------------------------------------------------------------------- the block
def _blocks(n, seed):
    """(two-switch block, _OwnDenseBlock on a deep copy) of n layers from 64 channels: kaiming weights as zoo.DenseNet's,
    BatchNorm statistics and affine maps randomised by the recipe of test_gpu_dense3x3.randomised_checkpoint (restated:
    gamma of both signs around 1, beta and mean 0.2 N(0,1), variance in [0.6, 1.4]); bf16, channels_last, on the device."""
    from dl_attack_on_imagenet_amd import zoo
    gen = torch.Generator().manual_seed(seed)
    r = lambda c: torch.randn(c, generator=gen)
    u = lambda c: torch.rand(c, generator=gen)
    sign = lambda c: (torch.randint(0, 2, (c,), generator=gen) * 2 - 1).float()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        block = zoo._DenseBlock(n, 64)
        for m in block.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight)
    block.eval()
    with torch.no_grad():
        for m in block.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_((0.7 + 0.6 * u(c)) * sign(c))
                m.bias.copy_(0.2 * r(c))
                m.running_mean.copy_(0.2 * r(c))
                m.running_var.copy_(0.6 + 0.8 * u(c))
    for p in block.parameters():
        p.requires_grad_(False)
    assert zoo.use_own_dense_pointwise_(block) == n and zoo.use_own_dense_conv_(block) == n
    two = block.to(device=DEV, dtype=BF16).to(memory_format=torch.channels_last)
    own = zoo._OwnDenseBlock(copy.deepcopy(two))
    return two, own


BLOCK_CASES = {"3-layers": (3, (2, 64, 9, 11)), "6-layers": (6, (1, 64, 16, 16))}


@pytest.fixture(scope="module")
def block_case():
    """The blocks, input and output gradient of each case, built once and left unchanged."""
    cache = {}

    def get(case):
        if case not in cache:
            n, shape = BLOCK_CASES[case]
            two, own = _blocks(n, 11 + n)
            gen = torch.Generator().manual_seed(100 + n)
            x = torch.randn(shape, generator=gen).to(BF16).to(DEV).contiguous(memory_format=torch.channels_last)
            g = torch.randn((shape[0], 64 + 32 * n) + shape[2:], generator=gen).to(BF16).to(DEV)
            cache[case] = (two, own, x, g.contiguous(memory_format=torch.channels_last))
        return cache[case]
    return get


@pytest.mark.parametrize("case", list(BLOCK_CASES), ids=str)
def test_block_forward_equals_the_two_switch_block_bitwise(block_case, monkeypatch, case):
    """The `_OwnDenseBlock` output equals the two-switch block's (torch.cat in front of every layer) bit for bit, with and
    without grad: only addresses changed.  The block path calls torch.cat zero times; the loop it replaces n + 1 times."""
    two, own, x, _ = block_case(case)
    n = len(own)
    with torch.no_grad():
        want = two(x)
        got = own(x)
    assert got.shape == want.shape == (x.shape[0], 64 + 32 * n) + x.shape[2:] and got.dtype == BF16
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert _same(got.permute(0, 2, 3, 1), want.permute(0, 2, 3, 1))
    assert _same(own(x.clone().requires_grad_(True)).detach().permute(0, 2, 3, 1), want.permute(0, 2, 3, 1))
    calls, real = [], torch.cat
    with monkeypatch.context() as mp:
        mp.setattr(torch, "cat", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        with torch.no_grad():
            own(x)
        assert len(calls) == 0
        own(x.clone().requires_grad_(True)).float().sum().backward()
        assert len(calls) == 0
        with torch.no_grad():
            two(x)
        assert len(calls) == n + 1


@pytest.mark.parametrize("case", list(BLOCK_CASES), ids=str)
def test_block_gradient_against_the_fp64_restatement(block_case, case):
    """Input gradient for a bf16 gaussian g against the fp64 restatement of the block (weights and tables upcast,
    activations unrounded): the relative error of the `_OwnDenseBlock` gradient (one fp32 add and one rounding per
    contribution, last layer first) is at most 1.5 x that of the two-switch block under autograd (every contribution
    rounded to bf16, then bf16 adds) — the factor of test_densenet_on_own_dense_conv_kernels; a wiring fault (wrong
    offset, missing accumulate, wrong xin) is off by order one.  g itself is unchanged by the backward.
    Recorded on an MI355X: relative error 0.04141 two-switch / 0.04140 block with 3 layers, 0.05712 / 0.05712 with 6."""
    two, own, x, g = block_case(case)
    _, ref = db.block_fp64(two, x, g)
    keep = g.clone()
    grads = []
    for block in (two, own):
        xin = x.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad(block(xin), xin, g)
        assert gx.shape == x.shape and gx.dtype == BF16
        grads.append(gx.detach().cpu().double())
    assert _same(g, keep)
    e_two, e_own = (float((gx - ref).norm() / ref.norm()) for gx in grads)
    print(case, "input-gradient relative error vs fp64: two-switch block %.5f, _OwnDenseBlock %.5f" % (e_two, e_own))
    assert float(ref.abs().max()) > 0 and e_own <= 1.5 * e_two, (e_two, e_own)


def test_block_in_a_captured_graph(block_case):
    """Forward + backward of the 3-layer block captured once in a graph on one stream: the replay on two input sets
    equals the eager result bit for bit (every launch on the capturing stream, no synchronisation, allocations from the
    allocator alone).  Modelled on test_dense3x3_in_a_captured_graph."""
    _, own, x0, g0 = block_case("3-layers")
    gen = torch.Generator().manual_seed(7)
    sets = [(x0, g0), (torch.randn(x0.shape, generator=gen).to(BF16).to(DEV), torch.randn(g0.shape, generator=gen).to(BF16).to(DEV))]

    def run(x, g):
        y = own(x)
        (gx,) = torch.autograd.grad(y, x, g)
        return y, gx

    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    eager = [tuple(t.detach().clone() for t in run(cl(x).clone().requires_grad_(True), cl(g))) for x, g in sets]
    xs = cl(x0).clone(memory_format=torch.preserve_format).requires_grad_(True)
    gs = cl(g0).clone(memory_format=torch.preserve_format)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(xs, gs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys, gxs = run(xs, gs)
    for (x, g), (want_y, want_gx) in zip(sets, eager):
        with torch.no_grad():
            xs.copy_(x)
            gs.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(ys.detach().permute(0, 2, 3, 1), want_y.permute(0, 2, 3, 1))
        assert _same(gxs.permute(0, 2, 3, 1), want_gx.permute(0, 2, 3, 1))


# ------------------------------------------------------------------------------------------------------------- network
def randomised_checkpoint(path, seed=5, num_classes=1000):
    """The recipe of tests/test_gpu_dense3x3.randomised_checkpoint (images None), restated: a seeded DenseNet-121
    state_dict with BatchNorm statistics drawn around the initial 0 / 1 and gamma of BOTH signs."""
    from dl_attack_on_imagenet_amd import zoo
    model = zoo.build_classifier("densenet121", num_classes=num_classes, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    r = lambda n: torch.randn(n, generator=gen)
    u = lambda n: torch.rand(n, generator=gen)
    sign = lambda n: (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_((0.7 + 0.6 * u(n)) * sign(n))
                m.bias.copy_(0.2 * r(n))
                m.running_mean.copy_(0.2 * r(n))
                m.running_var.copy_(0.6 + 0.8 * u(n))
    torch.save(model[1].state_dict(), path)
    return path


def _forward_and_gradient(model, x):
    x = x.clone().requires_grad_(True)
    logits = model(x).float()
    (g,) = torch.autograd.grad(logits.square().sum(), x)
    return logits.detach(), g.detach().float()


def test_densenet_on_the_dense_block_path(tmp_path, monkeypatch):
    """All three switches on 4 structured images at 64 x 64 and a checkpoint with randomised BatchNorm statistics (the
    fixture recipe of test_densenet_on_own_dense_conv_kernels, restated): the logits against the fp32 network within the
    bf16 depth bound of 121 layers, the input gradient no further from the fp32 network's than 1.5 x the distance of the
    plain bf16 network; 4 `_OwnDenseBlock`s; torch.cat is called 0 times and F.conv2d once (the stem) per forward; two
    fresh builds give bitwise equal logits and input gradients.
    Recorded on an MI355X: mean |logit error| 0.00537 plain bf16 / 0.00281 three switches, rms logit 0.6155, bound 0.02645;
    input-gradient relative error 0.1397 plain bf16 / 0.1314 three switches."""
    from structured import structured_images
    from dl_attack_on_imagenet_amd import zoo
    images, _ = structured_images(4, classes=4, seed=3, size=64)
    path = randomised_checkpoint(os.path.join(str(tmp_path), "densenet_random_bn.pt"))
    kw = dict(num_classes=1000, seed=5, weights=path, device=DEV)
    x = images.to(DEV)
    lr, gr = _forward_and_gradient(zoo.build_classifier("densenet121", **kw), x)
    kw.update(dtype=BF16, channels_last=True)
    l0, g0 = _forward_and_gradient(zoo.build_classifier("densenet121", **kw), x.bfloat16())
    rms = float(lr.square().mean().sqrt())
    bound = _bf16_depth_bound(121) * rms
    rel = lambda g: float((g - gr).norm() / gr.norm())
    e0, r0 = float((l0 - lr).abs().mean()), rel(g0)
    assert float(gr.abs().max()) > 0
    three = dict(own_dense_pointwise=True, own_dense_conv=True, own_dense_block=True)
    own = zoo.build_classifier("densenet121", **three, **kw)
    assert sum(isinstance(m, zoo._OwnDenseBlock) for m in own.modules()) == 4
    l1, g1 = _forward_and_gradient(own, x.bfloat16())
    e1, r1 = float((l1 - lr).abs().mean()), rel(g1)
    print("logit error vs fp32: plain bf16 %.5f three switches %.5f, rms %.4f, bound %.5f; input gradient relative error vs "
          "fp32: plain bf16 %.4f three switches %.4f" % (e0, e1, rms, bound, r0, r1))
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all() and g1.shape == x.shape and float(g1.abs().max()) > 0
    assert e1 <= bound, (e0, e1, rms)
    assert r1 <= 1.5 * r0, (r0, r1)
    cats, convs, real_cat, real_conv = [], [], torch.cat, F.conv2d
    with monkeypatch.context() as mp:
        mp.setattr(torch, "cat", lambda *a, **k: (cats.append(1), real_cat(*a, **k))[1])
        mp.setattr(F, "conv2d", lambda *a, **k: (convs.append(tuple(a[1].shape)), real_conv(*a, **k))[1])
        with torch.no_grad():
            own(x.bfloat16())
        assert cats == [] and convs == [(64, 3, 7, 7)], (len(cats), convs)
        _forward_and_gradient(own, x.bfloat16())
        assert cats == [], len(cats)
    again = zoo.build_classifier("densenet121", **three, **kw)
    l2, g2 = _forward_and_gradient(again, x.bfloat16())
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
