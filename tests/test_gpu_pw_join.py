"""GPU: the residual-join kernels (adil_pw_join_fwd / adil_pw_join_bwd) are bitwise the two pointwise kernels they
replace, at both widths the C ABI covers and at ragged pixel counts; the network with chained joins keeps the
fp32-reference accuracy of the unchained one, and the graphed learner step runs them under capture."""
import pytest
import torch

from graph_tools import assert_graph_used, no_capture_fallback, same_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _lib():
    from dl_attack_on_imagenet_amd import _lib as L
    return L.load()


def _ops():
    from dl_attack_on_imagenet_amd import ops
    return ops


def _join_operands(m, wd, seed):
    c = 4 * wd
    gen = torch.Generator().manual_seed(seed)
    bf = lambda *s, k=1.0: (torch.randn(*s, generator=gen) * k).bfloat16().to(DEV)
    return dict(
        h2raw=bf(m, wd), res=torch.relu(bf(m, c)), w3=bf(c, wd, k=wd ** -0.5), w1=bf(wd, c, k=c ** -0.5),
        ps2=(0.5 + torch.rand(wd, generator=gen)).to(DEV), pb2=(torch.randn(wd, generator=gen) * 0.3).to(DEV),
        s3=(0.5 + torch.rand(c, generator=gen)).to(DEV), b3=(torch.randn(c, generator=gen) * 0.3).to(DEV),
        s1=(0.5 + torch.rand(wd, generator=gen)).to(DEV), b1=(torch.randn(wd, generator=gen) * 0.3).to(DEV),
        g_h1=bf(m, wd), g_out=bf(m, c), h1=torch.relu(bf(m, wd)))


# ResNet-50 at B = 512: stage 1 (56x56, width 64) and stage 2 (28x28, width 128); then ragged pixel counts
SHAPES = [(512 * 56 * 56, 64), (512 * 28 * 28, 128), (1000, 64), (333, 128), (77, 64)]


@pytest.mark.parametrize("m,wd", SHAPES)
def test_join_forward_is_bitwise_the_two_pointwise_kernels(m, wd):
    lib, o = _lib(), _ops()
    t = _join_operands(m, wd, m + wd)
    c, p = 4 * wd, o._ptr
    out_a = torch.empty(m, c, dtype=torch.bfloat16, device=DEV)
    h1_a = torch.empty(m, wd, dtype=torch.bfloat16, device=DEV)
    assert lib.adil_pw_conv_fwd(p(t["h2raw"]), p(t["w3"]), p(t["s3"]), p(t["b3"]), p(t["res"]), p(out_a), m, wd, c, 1,
                                p(t["ps2"]), p(t["pb2"]), 0, 0, o._stream()) == 0
    assert lib.adil_pw_conv_fwd(p(out_a), p(t["w1"]), p(t["s1"]), p(t["b1"]), None, p(h1_a), m, c, wd, 1, None, None, 0, 0,
                                o._stream()) == 0
    out_b = torch.full((m + 1, c), 7.0, dtype=torch.bfloat16, device=DEV)
    h1_b = torch.full((m + 1, wd), 7.0, dtype=torch.bfloat16, device=DEV)
    assert lib.adil_pw_join_fwd(p(t["h2raw"]), p(t["ps2"]), p(t["pb2"]), p(t["w3"]), p(t["s3"]), p(t["b3"]), p(t["res"]),
                                p(out_b), p(t["w1"]), p(t["s1"]), p(t["b1"]), p(h1_b), m, wd, c, o._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out_b[:m].view(torch.int16), out_a.view(torch.int16))
    assert torch.equal(h1_b[:m].view(torch.int16), h1_a.view(torch.int16))
    assert bool((out_b[m:] == 7.0).all()) and bool((h1_b[m:] == 7.0).all())
    assert float(h1_a.float().abs().sum()) > 0                      # not a vacuous comparison


@pytest.mark.parametrize("m,wd", SHAPES)
def test_join_backward_is_bitwise_the_two_pointwise_kernels(m, wd):
    lib, o = _lib(), _ops()
    t = _join_operands(m, wd, 3 * m + wd)
    c, p = 4 * wd, o._ptr
    out = t["res"]                                                  # any ReLU output
    wt1, wt3 = t["w1"].t().contiguous(), t["w3"].t().contiguous()
    tt = torch.empty(m, c, dtype=torch.bfloat16, device=DEV)
    gres_a = torch.empty(m, c, dtype=torch.bfloat16, device=DEV)
    gx_a = torch.empty(m, wd, dtype=torch.bfloat16, device=DEV)
    assert lib.adil_pw_conv_bwd(p(t["g_h1"]), None, p(t["h1"]), p(t["s1"]), p(wt1), p(tt), None, m, c, wd, 1, None, None,
                                None, None, 0, 0, o._stream()) == 0
    assert lib.adil_pw_conv_bwd(p(tt), p(t["g_out"]), p(out), p(t["s3"]), p(wt3), p(gx_a), p(gres_a), m, wd, c, 1,
                                p(t["h2raw"]), p(t["ps2"]), p(t["pb2"]), None, 0, 0, o._stream()) == 0
    gres_b = torch.full((m + 1, c), 7.0, dtype=torch.bfloat16, device=DEV)
    gx_b = torch.full((m + 1, wd), 7.0, dtype=torch.bfloat16, device=DEV)
    assert lib.adil_pw_join_bwd(p(t["g_h1"]), p(t["h1"]), p(t["s1"]), p(wt1), p(t["g_out"]), p(out), p(t["s3"]), p(gres_b),
                                p(wt3), p(t["h2raw"]), p(t["ps2"]), p(t["pb2"]), p(gx_b), m, wd, c, o._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(gres_b[:m].view(torch.int16), gres_a.view(torch.int16))
    assert torch.equal(gx_b[:m].view(torch.int16), gx_a.view(torch.int16))
    assert bool((gres_b[m:] == 7.0).all()) and bool((gx_b[m:] == 7.0).all())
    assert float(gx_a.float().abs().sum()) > 0


def test_join_rejects_widths_it_does_not_cover():
    lib, o = _lib(), _ops()
    x = torch.zeros(4096, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(4096, device=DEV)
    p = o._ptr
    for wd, c in ((32, 128), (256, 1024), (512, 2048), (64, 128)):
        assert lib.adil_pw_join_fwd(p(x), p(f), p(f), p(x), p(f), p(f), p(x), p(x), p(x), p(f), p(f), p(x), 4, wd, c,
                                    o._stream()) == -1
        assert lib.adil_pw_join_bwd(p(x), p(x), p(f), p(x), p(x), p(x), p(f), p(x), p(x), p(x), p(f), p(f), p(x), 4, wd, c,
                                    o._stream()) == -1


def _resnet50(seed, **kw):
    from dl_attack_on_imagenet_amd import zoo
    model = zoo.build_classifier("resnet50", num_classes=10, seed=seed, device=DEV, dtype=torch.bfloat16, channels_last=True,
                                 fuse_bn_act=True, fuse_stem=True, **kw)
    (net,) = [m for m in model.modules() if isinstance(m, zoo.FusedResNet)]
    return model, net


def test_fused_resnet50_chained_joins_match_fp32():
    """The network is not bitwise reproducible from one call to the next even with unchained joins (its library
    convolutions are not: logits move by up to 0.125, measured), so the whole-network check is the fp32-reference bound
    of test_gpu_stem.test_fused_resnet50_gradient_matches_fp32 for both routes; the join kernels themselves are
    compared bitwise above."""
    import torch.nn.functional as F
    from dl_attack_on_imagenet_amd import zoo
    ref = zoo.build_classifier("resnet50", num_classes=10, seed=5, device=DEV, dtype=torch.float32)
    model, net = _resnet50(5)
    assert net.chain_joins and sum(net._join_next) == 2            # stage 1 (ops.JOIN_WIDTHS): 2 joins
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(0)).to(DEV).bfloat16()
    xr = x.float().requires_grad_(True)
    lr = ref(xr)
    (gr,) = torch.autograd.grad(lr.square().sum(), xr)
    rms = float(lr.square().mean().sqrt())
    cos = lambda a, b: float(F.cosine_similarity(a.float().flatten(), b.float().flatten(), dim=0))
    out = {}
    for on in (False, True):
        net.chain_joins = on
        xi = x.clone().requires_grad_(True)
        lo = model(xi).float()
        (g,) = torch.autograd.grad(lo.square().sum(), xi)
        out[on] = (float((lo - lr).abs().mean().detach()), cos(g, gr), float(g.float().norm()))
    net.chain_joins = True
    print("chain off / on: logit error %.4f / %.4f, gradient cosine %.5f / %.5f, rms(logits) %.3f"
          % (out[False][0], out[True][0], out[False][1], out[True][1], rms))
    nr = float(gr.norm())
    (e0, c0, n0), (e1, c1, n1) = out[False], out[True]
    assert e1 <= 0.03 * rms and e1 <= 1.5 * e0 + 0.01 * rms, (e0, e1, rms)
    assert c1 >= c0 - 0.01, (c0, c1)
    assert abs(n1 - nr) <= abs(n0 - nr) + 0.02 * nr, (n0, n1, nr)
    assert model(torch.rand(0, 3, 64, 64, device=DEV)).shape == (0, 10)     # empty batches pass through


def _graphed_against_eager(model, steps=8):
    """Two learners from one state on the same eight images, one through step, one through step_graphed: loss and fooled
    count per step and both learners afterwards."""
    from dl_attack_on_imagenet_amd import engine, ops
    g = torch.Generator().manual_seed(3)
    images = torch.rand(8, 3, 64, 64, generator=g).to(DEV)
    index = torch.arange(8, device=DEV)
    d0 = (-1 + 2 * torch.rand(3, 64, 64, 6, generator=g)).to(DEV)
    v0 = ops.l1ball_project_(torch.rand(8, 6, generator=g).to(DEV), 0.3)
    a = engine.DictionaryLearner(d0.clone(), v0.clone(), 0.3, 0.01, "logits")
    b = engine.DictionaryLearner(d0.clone(), v0.clone(), 0.3, 0.01, "logits")
    per_step = []
    with no_capture_fallback():
        for _ in range(steps):
            la, fa = a.step(model, images, index)
            lb, fb = b.step_graphed(model, images, index)
            per_step.append((la, fa, lb, fb))
    assert_graph_used(b)
    assert bool(torch.isfinite(b.d).all()) and not torch.equal(a.d, d0)
    return a, b, per_step


LEARNER_STATE = ("d", "v", "m_d", "s_d", "m_v", "s_v")


def test_graphed_step_with_chained_joins_matches_eager():
    """The join Functions under hipGraph capture and replay, bit for bit.  With own_strided_conv the network holds no library
    convolution and is bitwise reproducible (test_gpu_conv_s2.py), so the eager learner is an exact reference: loss and fooled
    count of each of 8 steps and d, v and the four moments afterwards are equal, and a graph was really recorded.
    Second leg, the build this test used before (library stride-2 convolutions): what it can show is the library's
    repeatability, not the joins; it runs under torch.backends.cudnn.deterministic like the library comparisons of
    test_gpu_conv_s2.py (profiles/graphed_classifiers.md has the eager-against-eager measurements behind its claim)."""
    model, net = _resnet50(7, own_strided_conv=True)
    assert net.chain_joins and sum(net._join_next) == 2            # stage 1 (ops.JOIN_WIDTHS): 2 joins
    assert net.own_strided_conv
    a, b, per_step = _graphed_against_eager(model)
    for step, (la, fa, lb, fb) in enumerate(per_step):
        same_state({"loss": la, "fooled": fa}, {"loss": lb, "fooled": fb}, ("loss", "fooled"))
    same_state(a, b, LEARNER_STATE)
    assert a.sched_d.t == b.sched_d.t == 8
    # the library leg
    model, net = _resnet50(7)
    assert net.chain_joins and sum(net._join_next) == 2 and not net.own_strided_conv
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        a, b, per_step = _graphed_against_eager(model)
    finally:
        torch.backends.cudnn.deterministic = prev
    for step, (la, fa, lb, fb) in enumerate(per_step):
        same_state({"loss": la, "fooled": fa}, {"loss": lb, "fooled": fb}, ("loss", "fooled"))
    same_state(a, b, LEARNER_STATE)
