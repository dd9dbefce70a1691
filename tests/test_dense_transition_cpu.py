"""CPU: host side of the pool-first transition kernels (adil_dense_transition_fwd / adil_dense_transition_bwd) and of the
two switches built on them: the built library exports the symbols, the header and the binding declare them, every refusal
returns before any device call; the fp32 emulation of the kernels against the restatement of
tests/dense_transition_reference.py on both legs of every row, with the premises asserted on the reference alone; the
comparators' power to reject the mutants; the restatement against torch's own BatchNorm, ReLU, convolution, average pool
and autograd in fp64 (the commuted form is the same function); `own_dense_transition`, `own_dense_stem`, their fallbacks
and the CLI defaults."""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dense1x1_reference as d1
import dense_transition_reference as tr
from classifier_reference import SCALES, Arith, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_and_header_declares_the_new_symbols():
    from dl_attack_on_imagenet_amd import _lib
    from dl_attack_on_imagenet_amd.build import build_library
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIBPATH)
    src = open(os.path.join(ROOT, "include", "adil_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in tr.NEW_SYMBOLS.items():
        assert hasattr(lib, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.load().adil_abi_version() == _lib.ABI_VERSION == 8


def test_refusals_need_no_device():
    """Each NULL, each misaligned pointer, K or N outside the limits, odd H, odd W, H = 0, B H W = 2^31, ldg below N or no
    multiple of 8: ADIL_EINVAL before any HIP call (the pointers are made-up addresses)."""
    from dl_attack_on_imagenet_amd import _lib
    lib = _lib.load()
    f = lambda x, ps, pb, w, y, B=2, H=4, W=4, K=64, N=32: lib.adil_dense_transition_fwd(x, ps, pb, w, y, B, H, W, K, N, None)
    b = lambda g, wt, xin, ps, pb, gx, ldg=32, B=2, H=4, W=4, K=64, N=32: lib.adil_dense_transition_bwd(
        g, ldg, wt, xin, ps, pb, gx, B, H, W, K, N, None)
    for i in range(5):
        null, odd = [16] * 5, [16] * 5
        null[i], odd[i] = None, (18 if i in (1, 2) else 24)          # tables: 4-byte alignment; bf16 operands: 16
        assert f(*null) == -1, i
        assert f(*odd) == -1, i
    for i in range(6):
        null, odd = [16] * 6, [16] * 6
        null[i], odd[i] = None, (18 if i in (3, 4) else 24)
        assert b(*null) == -1, i
        assert b(*odd) == -1, i
    dims = [dict(K=12), dict(N=20), dict(K=2056), dict(N=2056), dict(K=0), dict(N=0), dict(K=-8), dict(H=3), dict(W=5),
            dict(H=0), dict(W=0), dict(H=-2), dict(B=0), dict(B=-1), dict(B=2 ** 15, H=2 ** 8, W=2 ** 8),
            dict(B=2 ** 20, H=2 ** 20, W=2 ** 20)]
    for d in dims:
        assert f(16, 16, 16, 16, 16, **d) == -1, d
        assert b(16, 16, 16, 16, 16, 16, **dict(d, ldg=4096)) == -1, d
    for ldg in (24, 31, 33, 36, 0, -32):
        assert b(16, 16, 16, 16, 16, 16, ldg=ldg) == -1, ldg


@pytest.mark.parametrize("row", tr.ROWS, ids=str)
def test_emulation_passes_every_row(row):
    """The fp32 emulation (reduction in chunks of 16) equals the restatement bit for bit on the row's exact leg and stays
    under the gaussian bound; the premises (quantum 1/8, 2^23, branch and mixed-window shares, rounding share) are asserted
    on the reference alone inside `reference_row`."""
    name = tr.row_name(*row)
    exact, _ = tr.legs_of(row)
    r, y, gx = tr.emulate(row, exact)
    d1.compare_exact(name + "/fwd", y, r.fwd)
    d1.compare_exact(name + "/bwd", gx, r.bwd)
    r, y, gx = tr.emulate(row, "gaussian")
    rf, rb = d1.gaussian_ratio(y, r.fwd), d1.gaussian_ratio(gx, r.bwd)
    assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)


def test_table_and_legs():
    assert len(tr.ROWS) == 11 and len(set(tr.ROWS)) == 11
    assert sorted(set(tr.EXACT_LEG.values())) == ["clamp", "rounding"]
    for h, k, n in tr.NETWORK_TRANSITIONS:
        assert k == 2 * n and h % 2 == 0
    from dl_attack_on_imagenet_amd import zoo
    net = zoo.DenseNet(num_classes=4)
    got = [(m.conv.in_channels, m.conv.out_channels) for name, m in net.features.named_children() if name.startswith("transition")]
    assert got == [(k, n) for _, k, n in tr.NETWORK_TRANSITIONS]


def _share_changed(row, leg, mut):
    """On the reference alone: the share of the reference's outputs (forward, gradient) a mutant changes in bits."""
    r = tr.reference_row(row, leg)
    ref, mu, o = Arith(), Arith(mut=(mut,)), r.ops
    out = []
    for fn, args in ((tr.tr_fwd, (o.x, o.pscale, o.pshift, o.w)), (tr.tr_bwd, (o.g, o.wt, o.x, o.pscale, o.pshift))):
        one, two = d1.finish(ref, fn(ref, row, *args)), d1.finish(mu, fn(mu, row, *args))
        out.append(float((bits(one) != bits(two)).double().mean()))
    return out


def _rejected(row, leg, mut):
    """(forward rejected, gradient rejected) by the comparators the GPU test uses, on the fp32 emulation with the mutant."""
    r, y, gx = tr.emulate(row, leg, (mut,))
    out = []
    for got, o in ((y, r.fwd), (gx, r.bwd)):
        if leg == "gaussian":
            out.append(d1.gaussian_ratio(got, o) > 1.0)
            continue
        try:
            d1.compare_exact(mut, got, o)
            out.append(False)
        except AssertionError:
            out.append(True)
    return out


# mutant -> (row, leg, which outputs it must change: 0 = forward, 1 = gradient)
MUTANTS = {
    "conv_first": ((1, 2, 6, 24, 40), "rounding", (0,)),
    "pool_bf16": ((2, 16, 16, 96, 128), "rounding", (0,)),
    "no_quarter": ((3, 4, 6, 72, 136), "clamp", (0, 1)),
    "linear_window": ((1, 2, 6, 24, 40), "rounding", (0, 1)),
    "pooled_mask": ((3, 4, 6, 72, 136), "clamp", (1,)),
    "fma": ((2, 16, 18, 256, 128), "gaussian", (1,)),
    "k_tail": ((3, 4, 6, 72, 136), "clamp", (0, 1)),
}


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_comparators_reject_the_mutants(mut):
    """Each mutant changes at least 1 % of the reference's outputs on its row (shown on the reference alone: the fp64
    restatement with and without the mutant, both rounded once), the emulation with the mutant fails the row's comparator
    there, and the emulation without it passes."""
    row, leg, outs = MUTANTS[mut]
    if leg != "gaussian":
        share = _share_changed(row, leg, mut)
        for i in outs:
            assert share[i] >= 0.01, (mut, row, leg, share)
    else:
        # the gaussian leg has no single correct output: the mutant must leave the bound on at least 1 % of the outputs
        r, y, gx = tr.emulate(row, leg, (mut,))
        for i in outs:
            got, o = ((y, r.fwd), (gx, r.bwd))[i]
            ref = d1.expected(o)
            a = d1.acc_eps(o.S, o.n)
            bound = (2.0 ** -8 * (ref.abs() + a) + a).clamp_min(2.0 ** -126)
            assert float(((got.double() - ref).abs() > bound).double().mean()) >= 0.01, (mut, row)
    rej, clean = _rejected(row, leg, mut), _rejected(row, leg, "none")
    for i in outs:
        assert rej[i], (mut, row, leg, i)
    assert clean == [False, False]


def test_linear_window_is_the_same_on_a_single_window():
    """Why the table has a row with pooled rows of 3: on a 2 x 2 image the linear window IS the window."""
    assert torch.equal(tr.windows(1, 2, 2), tr.windows(1, 2, 2, linear=True))
    assert not torch.equal(tr.windows(1, 2, 6), tr.windows(1, 2, 6, linear=True))
    idx = tr.windows(3, 4, 6)
    assert sorted(idx.flatten().tolist()) == list(range(3 * 4 * 6))    # every input pixel in exactly one window


@pytest.mark.parametrize("dims", [(2, 4, 6, 24, 40), (1, 2, 2, 8, 8), (3, 6, 4, 72, 16)], ids=str)
def test_restatement_equals_torch(dims):
    """In fp64 and without any rounding, the commuted form (pool, then convolve) equals torch's
    avg_pool2d(conv2d(relu(batch_norm(x)), w), 2) and its autograd input gradient to 1e-12 relative: the same function."""
    from dl_attack_on_imagenet_amd import zoo
    B, H, W, K, N = dims
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B * H * W, K, generator=gen, dtype=torch.float64)
    g = torch.randn(B * (H // 2) * (W // 2), N, generator=gen, dtype=torch.float64)
    w = torch.randn(N, K, generator=gen, dtype=torch.float64)
    bn = torch.nn.BatchNorm2d(K, eps=2.0 ** -10).double().eval()
    with torch.no_grad():
        bn.running_var.fill_(1.0 - 2.0 ** -10)                        # var + eps = 1 exactly: the affine map is (weight, bias)
        bn.running_mean.zero_()
        bn.weight.copy_(torch.tensor(SCALES, dtype=torch.float64)[torch.randint(0, len(SCALES), (K,), generator=gen)])
        bn.bias.copy_(torch.randint(-4, 5, (K,), generator=gen).double())
    ps, pb = zoo._bn_affine(bn)
    assert torch.equal(ps.double(), bn.weight) and torch.equal(pb.double(), bn.bias)
    ar = Arith(mut=("unrounded",))
    fwd = tr.tr_fwd(ar, dims, x, ps, pb, w)
    bwd = tr.tr_bwd(ar, dims, g, w.t().contiguous(), x, ps, pb)
    nchw = lambda t, h, wd: t.reshape(B, h, wd, -1).permute(0, 3, 1, 2)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    xin = nchw(x, H, W).clone().requires_grad_(True)
    act = torch.relu(F.batch_norm(xin, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps))
    yref = F.avg_pool2d(F.conv2d(act, w.reshape(N, K, 1, 1)), 2)
    (gxref,) = torch.autograd.grad(yref, xin, nchw(g, H // 2, W // 2))
    assert float((d1.expected(fwd) - flat(yref.detach())).abs().max()) <= 1e-12 * (1 + float(yref.detach().abs().max()))
    assert float((d1.expected(bwd) - flat(gxref)).abs().max()) <= 1e-12 * (1 + float(gxref.abs().max()))


# ----------------------------------------------------------------------------------------------------------- the switches
SWITCHES = dict(dtype=torch.bfloat16, channels_last=True, own_dense_pointwise=True, own_dense_conv=True, own_dense_block=True,
                own_dense_transition=True, own_dense_stem=True, num_classes=8)


def test_rewrites_return_their_counts_and_keep_the_state_dict():
    from dl_attack_on_imagenet_amd import zoo
    torch.manual_seed(0)
    plain = zoo.DenseNet(num_classes=8).eval()
    own = copy.deepcopy(plain)
    assert zoo.use_own_dense_transition_(own) == 0                 # no _OwnTransition yet: nothing to switch
    assert zoo.use_own_dense_pointwise_(own) == 61
    assert not any(m.pool_first for m in own.modules() if isinstance(m, zoo._OwnTransition))
    assert zoo.use_own_dense_transition_(own) == 3
    assert all(m.pool_first for m in own.modules() if isinstance(m, zoo._OwnTransition))
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    assert zoo.use_own_dense_stem_(own, mean, std) == 1
    assert isinstance(own.features, zoo._OwnDenseStem) and isinstance(own.features, torch.nn.Sequential)
    assert [n for n, _ in own.features.named_children()] == [n for n, _ in plain.features.named_children()]
    sd0, sd1 = plain.state_dict(), own.state_dict()
    assert list(sd0.keys()) == list(sd1.keys())
    assert all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    buffers = dict(own.features.named_buffers(recurse=False))
    assert sorted(buffers) == ["norm_mean", "norm_std", "scale", "shift", "w_bwd", "w_fwd"]
    own.bfloat16()                                                 # the tables stay fp32, the rest is cast with the network
    assert own.features.scale.dtype == own.features.shift.dtype == torch.float32
    assert own.features.w_fwd.dtype == own.features.norm_mean.dtype == torch.bfloat16
    with pytest.raises(ValueError, match="own_dense_stem rewrites"):
        zoo.use_own_dense_stem_(zoo.ResNet(zoo.BasicBlock, [1, 1, 1, 1], num_classes=4), mean, std)
    with pytest.raises(ValueError, match="own_dense_stem rewrites"):
        zoo.use_own_dense_stem_(own, mean, std)                   # already rewritten: `features` is no plain stem any more


def test_fallbacks_are_the_plain_network_bit_for_bit():
    """Built with every switch on and run on the CPU (bf16), or moved back to fp32, the network is the network without
    switches, bit for bit: every rewritten module falls back to its children, and the stem module normalises operation for
    operation as `Normalize` does.  The state_dict keys are the plain network's."""
    from dl_attack_on_imagenet_amd import zoo
    own = zoo.build_classifier("densenet", **SWITCHES)
    plain = zoo.build_classifier("densenet", dtype=torch.bfloat16, channels_last=True, num_classes=8)
    assert len(own) == 1 and len(plain) == 2                       # the stem module took the normalisation over
    assert isinstance(own[0].features, zoo._OwnDenseStem)
    assert sum(m.pool_first for m in own.modules() if isinstance(m, zoo._OwnTransition)) == 3
    assert list(own[0].state_dict().keys()) == list(plain[1].state_dict().keys())
    fp32 = zoo.build_classifier("densenet", num_classes=8)
    assert list(own[0].state_dict().keys()) == list(fp32[1].state_dict().keys())
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        assert torch.equal(own(x.bfloat16()), plain(x.bfloat16()))
        own, plain = own.float(), plain.float()
        assert torch.equal(own(x), plain(x))
        odd = torch.rand(1, 3, 33, 35, generator=torch.Generator().manual_seed(4))
        assert torch.equal(own(odd), plain(odd))


def test_transition_routing_conditions(monkeypatch):
    """`ops.dense_transition_covers` adds an even H and W (>= 2) to the limits of the 1x1 kernels; an `_OwnTransition`
    pools first only with the switch on and an AvgPool2d(2, 2) without padding or ceil_mode.  The device test is patched
    out: no GPU is needed to decide on shapes."""
    from dl_attack_on_imagenet_amd import ops, zoo
    x = lambda h, w, c=64: torch.zeros(1, c, h, w, dtype=torch.bfloat16)
    assert not ops.dense_transition_covers(x(4, 4), 64, 32)        # a CPU tensor
    t = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError, match="does not cover"):
        ops.dense_transition(x(4, 4), t(64), t(64), t(32, 64).bfloat16(), t(64, 32).bfloat16())
    with pytest.raises(ValueError, match="w2d must be"):
        ops.dense_transition(x(4, 4), t(64), t(64), t(32, 64, 1, 1).bfloat16(), t(64, 32).bfloat16())
    monkeypatch.setattr(ops, "dense1x1_covers", lambda x, cin, cout: x.shape[1] == cin)
    assert ops.dense_transition_covers(x(4, 6), 64, 32)
    for h, w in ((5, 4), (4, 7), (1, 4), (4, 1), (3, 3)):
        assert not ops.dense_transition_covers(x(h, w), 64, 32), (h, w)
    net = zoo.DenseNet(num_classes=4).eval()
    zoo.use_own_dense_pointwise_(net)
    tr1 = net.features.transition1
    assert not tr1._pools_first(x(4, 4, 256))                      # the switch is off
    zoo.use_own_dense_transition_(net)
    assert tr1._pools_first(x(4, 4, 256))
    assert not tr1._pools_first(x(5, 4, 256)) and not tr1._pools_first(x(4, 3, 256))      # odd H, odd W: today's path
    for pool in (torch.nn.MaxPool2d(2, 2), torch.nn.AvgPool2d(3, 2, 1), torch.nn.AvgPool2d(2, 2, ceil_mode=True),
                 torch.nn.AvgPool2d(2, 1), torch.nn.AvgPool2d(2, 2, divisor_override=3)):
        tr1.pool = pool
        assert not tr1._pools_first(x(4, 4, 256)), pool
    tr1.pool = torch.nn.AvgPool2d((2, 2), (2, 2))
    assert tr1._pools_first(x(4, 4, 256))


def test_strided_gradient_view_is_taken_in_place():
    """`ops._strided_rows`: a contiguous channels_last gradient and the first N channels of a wider channels_last buffer
    are passed as they are with their row pitch; a pitch that is no multiple of 8, another dtype, a misaligned start or an
    NCHW-contiguous gradient take the one copy of `_nhwc_grad`."""
    from dl_attack_on_imagenet_amd import ops
    buf = torch.zeros(2, 3, 4, 40, dtype=torch.bfloat16)               # NHWC storage, 40 channels
    nchw = buf.permute(0, 3, 1, 2)
    g2, ld = ops._strided_rows(nchw, 40)
    assert ld == 40 and g2.data_ptr() == buf.data_ptr()
    g2, ld = ops._strided_rows(nchw[:, :16], 16)
    assert ld == 40 and g2.data_ptr() == buf.data_ptr() and tuple(g2.shape) == (2, 3, 4, 16)
    g2, ld = ops._strided_rows(nchw[:, 4:20], 16)                      # starts 8 bytes into a row: misaligned
    assert ld == 16 and g2.is_contiguous() and g2.data_ptr() != buf[..., 4:].data_ptr()
    odd = torch.zeros(2, 3, 4, 36, dtype=torch.bfloat16).permute(0, 3, 1, 2)[:, :16]
    g2, ld = ops._strided_rows(odd, 16)                                # pitch 36: no multiple of 8
    assert ld == 16 and g2.is_contiguous()
    g2, ld = ops._strided_rows(nchw[:, :16].float(), 16)
    assert ld == 16 and g2.dtype == torch.bfloat16 and g2.is_contiguous()
    g2, ld = ops._strided_rows(torch.zeros(2, 16, 3, 4, dtype=torch.bfloat16), 16)
    assert ld == 16 and g2.is_contiguous() and tuple(g2.shape) == (2, 3, 4, 16)


def test_build_classifier_switches():
    from dl_attack_on_imagenet_amd import zoo
    with pytest.raises(ValueError, match="own_dense_transition is a switch of DenseNet-121"):
        zoo.build_classifier("resnet18", dtype=torch.bfloat16, channels_last=True, own_dense_transition=True, num_classes=8)
    with pytest.raises(ValueError, match="own_dense_stem is a switch of DenseNet-121"):
        zoo.build_classifier("mobilenet", dtype=torch.bfloat16, channels_last=True, own_dense_stem=True, num_classes=8)
    with pytest.raises(ValueError, match="own_dense_transition needs own_dense_pointwise=True"):
        zoo.build_classifier("densenet121", dtype=torch.bfloat16, channels_last=True, own_dense_transition=True, num_classes=8)
    with pytest.raises(ValueError, match="own_dense_stem needs a bfloat16 network"):
        zoo.build_classifier("densenet121", channels_last=True, own_dense_stem=True, num_classes=8)
    with pytest.raises(ValueError, match="own_dense_stem needs channels_last=True"):
        zoo.build_classifier("densenet121", dtype=torch.bfloat16, own_dense_stem=True, num_classes=8)
    with pytest.raises(ValueError, match="needs a bfloat16 network"):
        zoo.build_classifier("densenet121", **dict(SWITCHES, dtype=torch.float32))
    with pytest.raises(ValueError, match="needs channels_last=True"):
        zoo.build_classifier("densenet121", **dict(SWITCHES, channels_last=False))
    # each new switch alone (the transition switch with the one it needs)
    stem = zoo.build_classifier("densenet", dtype=torch.bfloat16, channels_last=True, own_dense_stem=True, num_classes=8)
    assert len(stem) == 1 and isinstance(stem[0].features, zoo._OwnDenseStem)
    assert not any(isinstance(m, zoo._OwnTransition) for m in stem.modules())
    trn = zoo.build_classifier("densenet", dtype=torch.bfloat16, channels_last=True, own_dense_pointwise=True,
                               own_dense_transition=True, num_classes=8)
    assert len(trn) == 2 and not isinstance(trn[1].features, zoo._OwnDenseStem)
    assert sum(m.pool_first for m in trn.modules() if isinstance(m, zoo._OwnTransition)) == 3
    off = zoo.build_classifier("densenet", dtype=torch.bfloat16, channels_last=True, own_dense_pointwise=True, num_classes=8)
    assert not any(m.pool_first for m in off.modules() if isinstance(m, zoo._OwnTransition))      # off by default


def test_cli_switches_default_to_off():
    import demo_dL_attack
    import main
    for mod in (demo_dL_attack, main):
        p = mod.build_parser()
        for flag, dest in (("--own-dense-transition", "own_dense_transition"), ("--own-dense-stem", "own_dense_stem")):
            assert getattr(p.parse_args([]), dest) == 0
            assert getattr(p.parse_args([flag, "1"]), dest) == 1
