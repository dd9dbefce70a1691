"""adil_maxpool_fwd and adil_stem_pool_bwd through the C ABI, and the stem chain `ops.resnet_stem`, against the restatements
of tests/stem_pool_reference.py and tests/classifier_reference.py.

kernel rows   p bit for bit (NaN as NaN), idx byte for byte, gy bit for bit wherever the fp32 sum is exact in any order
              (zeros as values), on an exact leg (integer gradients in [-255, 255], scales +-1/2 .. +-2 times 1 or 1.5: the
              final rounding really rounds, ties occur) and a gaussian leg.  An element off the exact-sum premise takes
              2^-8 (|r| + A) + A, A = 4 2^-24 S |scale|; tests/test_stem_pool_cpu.py caps them at 1e-4 of a row.
              p, idx and gy lie between canaries; gy is prefilled with NaN and every element must be written.
the chain     exact leg: the pooled output equals maxpool_fwd(finish(stem_fwd)) bit for bit and the input gradient equals
              stem_bwd(pool_bwd(g)) bit for bit, for a channels_last bf16 g, an NCHW fp32 g and a non-contiguous x.
              gaussian leg: every p within the largest bound of its window's taps (the maximum is 1-Lipschitz), gx within
              stem_bwd's bound from the restated gy.  Nothing measured enters a bound.

Recorded on an MI355X (max |err| / bound, worst of the six rows each): chain forward 0.964 (the bf16 rounding of p alone
reaches 1 just above a power of two), chain backward 0.924 for a bf16 gx and 0.001 for an fp32 gx.  gy elements that took
the bound: 3 of 802816 in 1x112x112x64-relu [gaussian], worst ratio 0.761; none in any other row.  Exact leg of gy: 4.45 % of
the elements really rounded and 2.51 % exact ties at 3x17x23x64-relu, 4.01 % and 2.28 % at 1x112x112x64-relu."""
from ctypes import c_float, c_void_p

import pytest
import torch

import classifier_reference as R
import stem_pool_reference as P
from classifier_reference import BF16, F32, Route

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
LEGS = ("exact", "gaussian")
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def lib():
    from dl_attack_on_imagenet_amd import _lib
    return _lib.load()


def ops():
    from dl_attack_on_imagenet_amd import ops as o
    return o


def ptr(t):
    return c_void_p(0 if t is None else t.data_ptr())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _code(dt):
    return 0 if dt == F32 else 1


class Guarded:
    """An output tensor filled with `fill`, between two runs of canary elements."""
    PAD = 512                                # elements: keeps the tensor 16-byte aligned for every dtype used here

    def __init__(self, shape, dtype=BF16, fill=P.CANARY, canary=P.CANARY):
        n = 1
        for s in shape:
            n *= s
        self.n, self.fill, self.canary = n, fill, canary
        self.buf = torch.full((n + 2 * self.PAD,), canary, dtype=dtype, device=DEV)
        self.t = self.buf[self.PAD:self.PAD + n].view(shape)
        self.t.fill_(fill)

    def intact(self):
        return bool((self.buf[:self.PAD] == self.canary).all()) and bool((self.buf[self.PAD + self.n:] == self.canary).all())

    def untouched(self):
        same = torch.isnan(self.t) if self.fill != self.fill else self.t == self.fill
        return self.intact() and bool(same.all())


def pool_fwd(L, y, p, idx, B, OH, OW, C):
    rc = L.adil_maxpool_fwd(ptr(y), ptr(p), ptr(idx), B, OH, OW, C, stream())
    torch.cuda.synchronize()
    return rc


def pool_bwd(L, g, idx, p, scale, gy, B, OH, OW, C):
    rc = L.adil_stem_pool_bwd(ptr(g), ptr(idx), ptr(p), ptr(scale), ptr(gy), B, OH, OW, C, stream())
    torch.cuda.synchronize()
    return rc


# ---------------------------------------------------------------------------------------------------------- kernel rows
@pytest.mark.parametrize("row", P.ROWS, ids=lambda r: r.name)
def test_pool_kernels(row):
    """Both legs of one row: return codes, p and idx against the restatement, canaries, every gy element written, gy bit for
    bit on the premise and within the bound off it.  The backward is fed the kernel's own p and idx, which the asserts
    before it make the restatement's."""
    L = lib()
    B, OH, OW, C = row.shape
    pshape = (B, P.pooled(OH), P.pooled(OW), C)
    for leg in LEGS:
        name = f"{row.name} [{leg}]"
        o = {k: v.to(DEV) for k, v in P.operands(row, leg).items()}
        if "y" in o:
            p, idx = Guarded(pshape), Guarded(pshape, torch.uint8, P.IDX_CANARY, P.IDX_CANARY)
            assert pool_fwd(L, o["y"], p.t, idx.t, B, OH, OW, C) == 0, name
            want_p, want_idx = P.maxpool_fwd(o["y"])
            P.same_selection(name, p.t, idx.t, want_p, want_idx, OH, OW)
            assert p.intact() and idx.intact(), f"{name}: a canary of p or idx was overwritten"
            p_in, idx_in = p.t, idx.t
        else:
            p_in, idx_in = o["p"], o["idx"]
            want_p, want_idx = p_in.float(), idx_in
        gy = Guarded((B, OH, OW, C), fill=float("nan"))
        assert pool_bwd(L, o["g"], idx_in, p_in, o["scale"], gy.t, B, OH, OW, C) == 0, name
        assert gy.intact(), f"{name}: a canary of gy was overwritten"
        assert not bool(torch.isnan(gy.t).any()), f"{name}: {int(torch.isnan(gy.t).sum())} elements of gy were not written"
        ref = P.pool_bwd(o["g"], want_idx, want_p, o["scale"], OH, OW)
        rep = P.compare_gy(name, gy.t, ref, leg == "exact")
        line = f"{name}: {rep.off_premise} of {rep.elements} gy elements off the premise, worst ratio {rep.worst_ratio:.3f}"
        if leg == "exact":
            line += "; non-zero %.1f %%, really rounded %.2f %%, exact ties %.2f %%" % tuple(100 * v for v in P.rounding_stats(ref))
        print(line)


def _need(gb):
    free, _ = torch.cuda.mem_get_info()
    if free < gb * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.0f} GB free, the test needs {gb} GB")


def test_pool_beyond_2_31_elements():
    """y and gy of [257][64][64][2048] hold more than 2^31 elements; the first image, the image that ends at element 2^31 and
    the last image, which begins there, against the restatement run on those images alone (exact leg)."""
    _need(14)
    L = lib()
    B, OH, OW, C = 257, 64, 64, 2048
    img = OH * OW * C
    assert B * img > 2 ** 31 and 255 * img < 2 ** 31 <= 256 * img
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    y = torch.empty(B, OH, OW, C, dtype=BF16, device=DEV)
    for b0 in range(0, B, 32):
        y[b0:b0 + 32].normal_(generator=gen).relu_()
    pshape = (B, P.pooled(OH), P.pooled(OW), C)
    p = torch.empty(pshape, dtype=BF16, device=DEV)
    idx = torch.empty(pshape, dtype=torch.uint8, device=DEV)
    g = torch.randint(-255, 256, pshape, generator=gen, device=DEV, dtype=torch.int16).to(BF16)
    scale = (R.Gen("big-pool", "exact").scale(C) * torch.where(torch.arange(C) % 2 == 0, 1.5, 1.0)).to(DEV)
    gy = torch.empty(B, OH, OW, C, dtype=BF16, device=DEV)
    images = (0, 255, 256)
    for i in images:
        gy[i].fill_(float("nan"))
    assert pool_fwd(L, y, p, idx, B, OH, OW, C) == 0
    assert pool_bwd(L, g, idx, p, scale, gy, B, OH, OW, C) == 0
    for i in images:
        name = f"beyond 2^31, image {i}"
        want_p, want_idx = P.maxpool_fwd(y[i:i + 1])
        P.same_selection(name, p[i:i + 1], idx[i:i + 1], want_p, want_idx, OH, OW)
        assert not bool(torch.isnan(gy[i]).any()), name
        rep = P.compare_gy(name, gy[i:i + 1], P.pool_bwd(g[i:i + 1], want_idx, want_p, scale, OH, OW), True)
        assert rep.off_premise == 0


# ------------------------------------------------------------------------------------------------------------ refusals
def _refused(fn, *outs):
    rc = fn()
    torch.cuda.synchronize()
    assert rc == EINVAL, rc
    for c in outs:
        assert c.untouched(), "a refused call wrote to its output"


def test_pool_refusals_leave_outputs_untouched():
    """ADIL_EINVAL before any launch: C % 8 != 0, a zero or negative size, each NULL pointer, for both pool entry points."""
    L = lib()
    B, OH, OW, C = 2, 4, 4, 16
    pshape = (B, 2, 2, C)
    y = torch.zeros(B, OH, OW, C, dtype=BF16, device=DEV)
    g, pin = torch.ones(pshape, dtype=BF16, device=DEV), torch.ones(pshape, dtype=BF16, device=DEV)
    iin = torch.full(pshape, 4, dtype=torch.uint8, device=DEV)
    scale = torch.ones(C, device=DEV)
    p, idx, gy = Guarded(pshape), Guarded(pshape, torch.uint8, P.IDX_CANARY, P.IDX_CANARY), Guarded((B, OH, OW, C))
    for dims in ((B, OH, OW, 12), (B, OH, OW, 4), (B, OH, OW, 0), (B, OH, OW, -8), (0, OH, OW, C), (-1, OH, OW, C), (B, 0, OW, C),
                 (B, -2, OW, C), (B, OH, 0, C), (B, OH, -2, C)):
        _refused(lambda: L.adil_maxpool_fwd(ptr(y), ptr(p.t), ptr(idx.t), *dims, stream()), p, idx)
        _refused(lambda: L.adil_stem_pool_bwd(ptr(g), ptr(iin), ptr(pin), ptr(scale), ptr(gy.t), *dims, stream()), gy)
    for args in ((None, p.t, idx.t), (y, None, idx.t), (y, p.t, None)):
        _refused(lambda: L.adil_maxpool_fwd(*(ptr(a) for a in args), B, OH, OW, C, stream()), p, idx)
    for args in ((None, iin, pin, scale, gy.t), (g, None, pin, scale, gy.t), (g, iin, None, scale, gy.t), (g, iin, pin, None, gy.t),
                 (g, iin, pin, scale, None)):
        _refused(lambda: L.adil_stem_pool_bwd(*(ptr(a) for a in args), B, OH, OW, C, stream()), gy)
    # and the accepted call writes: the canaries above are no dead memory
    assert pool_fwd(L, y, p.t, idx.t, B, OH, OW, C) == 0 and not p.untouched() and p.intact()


def _stem_fwd_call(L, o, y, B, H, W, code):
    rc = L.adil_stem_conv_fwd(ptr(o["x"]), code, ptr(o["_wf"]), *(c_float(v) for v in o["mean"]), *(c_float(v) for v in o["inv_std"]),
                              ptr(o["scale"]), ptr(o["shift"]), ptr(y), B, H, W, stream())
    torch.cuda.synchronize()
    return rc


def _stem_bwd_call(L, o, gx, B, H, W, code):
    rc = L.adil_stem_conv_bwd(ptr(o["gy"]), ptr(o["_wb"]), *(c_float(v) for v in o["inv_std"]), ptr(gx), code, B, H, W, stream())
    torch.cuda.synchronize()
    return rc


def _stem_operands(family, B, H, W, dt, leg="exact"):
    o = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v)
         for k, v in R.operands(Route(family, "", dict(B=B, H=H, W=W, dtype=dt)), leg).items()}
    o["_wf" if family == "stem_fwd" else "_wb"] = (R.pack_stem_fwd if family == "stem_fwd" else R.pack_stem_bwd)(o["w"]).contiguous()
    return o


def test_stem_conv_refusals_leave_outputs_untouched():
    """ADIL_EINVAL before any launch: odd H or W, a dtype code outside the two, and B = 65536 (the image index is a grid
    dimension; before the guard the outcome was the runtime's: a launch error code where it caps gridDim.z at 65535, a
    launch and return code 0 where it does not, as recorded on an MI355X)."""
    L = lib()
    for B, H, W, code in ((2, 3, 4, 0), (2, 4, 6 + 1, 1), (2, 4, 4, 2), (2, 4, 4, -1), (65536, 2, 2, 0), (65536, 2, 2, 1)):
        dt = BF16 if code == 1 else F32
        hh, ww = max(H // 2, 1), max(W // 2, 1)
        f = dict(x=torch.zeros(B, 3, H, W, dtype=dt, device=DEV), _wf=torch.zeros(64, 224, dtype=BF16, device=DEV), mean=(0.0,) * 3,
                 inv_std=(1.0,) * 3, scale=torch.ones(64, device=DEV), shift=torch.zeros(64, device=DEV))
        y = Guarded((B, hh, ww, 64))
        _refused(lambda: _stem_fwd_call(L, f, y.t, B, H, W, code), y)
        b = dict(gy=torch.zeros(B, hh, ww, 64, dtype=BF16, device=DEV), _wb=torch.zeros(4, 49 * 64, dtype=BF16, device=DEV),
                 inv_std=(1.0,) * 3)
        gx = Guarded((B, 3, H, W), dt)
        _refused(lambda: _stem_bwd_call(L, b, gx.t, B, H, W, code), gx)
    o = ops()
    z = torch.zeros(64, device=DEV)
    with pytest.raises(ValueError, match="65535"):
        o.resnet_stem(torch.zeros(65536, 3, 2, 2, device=DEV), torch.zeros(64, 224, dtype=BF16, device=DEV),
                      torch.zeros(4, 49 * 64, dtype=BF16, device=DEV), z, z, (0.0,) * 3, (1.0,) * 3)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["float32", "bfloat16"])
def test_stem_convs_at_the_largest_admitted_batch(dt):
    """B = 65535, H = W = 2 through both stem convolutions on the exact leg, bit for bit: the largest admitted grid is whole."""
    L = lib()
    B, H, W = 65535, 2, 2
    o = _stem_operands("stem_fwd", B, H, W, dt)
    ref = R.stem_fwd(R.Arith(), **{k: v for k, v in o.items() if not k.startswith("_")})["y"]
    y = Guarded((B, 1, 1, 64))
    assert _stem_fwd_call(L, o, y.t, B, H, W, _code(dt)) == 0
    R.compare_exact(f"stem_fwd B={B} {dt}", y.t, ref)
    assert y.intact()
    b = _stem_operands("stem_bwd", B, H, W, dt)
    refb = R.stem_bwd(R.Arith(), **{k: v for k, v in b.items() if not k.startswith("_")})["gx"]
    gx = Guarded((B, 3, H, W), dt)
    assert _stem_bwd_call(L, b, gx.t, B, H, W, _code(dt)) == 0
    R.compare_exact(f"stem_bwd B={B} {dt}", gx.t, refb)
    assert gx.intact()


# ----------------------------------------------------------------------------------------------------------- the chain
CHAIN = [(2, 32, 64), (2, 20, 36), (1, 70, 38)]           # pooled grids 8 x 16, 5 x 9, 18 x 10
CHAIN_ROWS = [pytest.param(s, dt, id="%dx%dx%d-%s" % (*s, "float32" if dt == F32 else "bfloat16")) for s in CHAIN for dt in (F32, BF16)]


def _chain(o, x):
    wf, wb = ops().pack_stem_weights(o["w"])
    return ops().resnet_stem(x, wf, wb, o["scale"], o["shift"], o["mean"], o["inv_std"])


def _forward_reference(o):
    return R.stem_fwd(R.Arith(), o["x"], o["w"], o["mean"], o["inv_std"], o["scale"], o["shift"])["y"]


def _check_layout(out, B, PH, PW):
    assert out.dtype == BF16 and tuple(out.shape) == (B, 64, PH, PW)
    assert out.permute(0, 2, 3, 1).is_contiguous(), "the pooled activation is not in channels_last storage"


@pytest.mark.parametrize("shape,dt", CHAIN_ROWS)
def test_chain_exact(shape, dt):
    """Forward and input gradient of ops.resnet_stem, bit for bit."""
    B, H, W = shape
    OH, OW = H // 2, W // 2
    PH, PW = P.pooled(OH), P.pooled(OW)
    name = f"chain {B}x{H}x{W} {dt} [exact]"
    o = _stem_operands("stem_fwd", B, H, W, dt)
    fo = _forward_reference(o)
    R.assert_premise(name + " y1", fo)
    want_p, want_idx = P.maxpool_fwd(R.finish(R.Arith(), fo))
    x = o["x"].clone().requires_grad_(True)
    out = _chain(o, x)
    _check_layout(out, B, PH, PW)
    assert x.dtype == dt
    saved_p, saved_idx = out.grad_fn.saved_tensors[:2]
    P.same_selection(name, out.detach().permute(0, 2, 3, 1), saved_idx, want_p, want_idx, OH, OW)
    # backward: integer g in [-8, 8]
    gn = torch.randint(-8, 9, (B, PH, PW, 64), generator=P.rng(name, "g")).to(BF16).to(DEV)
    gyr = P.pool_bwd(gn, want_idx, want_p, o["scale"], OH, OW)
    assert bool(gyr.exact_sum.all())
    want_gx = R.stem_bwd(R.Arith(), gyr.want, o["w"], o["inv_std"], H, W, dt)["gx"]
    g_cl = gn.permute(0, 3, 1, 2)                                       # channels_last bf16: the no-copy path of _nhwc_grad
    assert g_cl.permute(0, 2, 3, 1).is_contiguous() and g_cl.dtype == BF16
    (gx,) = torch.autograd.grad(out, x, g_cl, retain_graph=True)
    assert gx.dtype == dt and gx.shape == x.shape
    R.compare_exact(name + " gx, channels_last bf16 g", gx, want_gx)
    g32 = (gn.float() * (1 + 2.0 ** -10)).permute(0, 3, 1, 2).contiguous()   # NCHW fp32, off the bf16 grid: cast and copy
    assert torch.equal(P.bf16_rne(g32), gn.float().permute(0, 3, 1, 2)) and not torch.equal(g32, gn.float().permute(0, 3, 1, 2))
    (gx32,) = torch.autograd.grad(out, x, g32)
    R.compare_exact(name + " gx, NCHW fp32 g", gx32, want_gx)
    # a non-contiguous x
    base = torch.full((B, 3, H, W + 6), 3.0, dtype=dt, device=DEV)
    base[..., 3:W + 3] = o["x"]
    base.requires_grad_(True)
    xv = base[..., 3:W + 3]
    assert not xv.is_contiguous()
    out_v = _chain(o, xv)
    _check_layout(out_v, B, PH, PW)
    assert torch.equal(R.bits(out_v.detach()), R.bits(out.detach()))
    (gb,) = torch.autograd.grad(out_v, base, g_cl)
    assert gb.dtype == dt and gb.shape == base.shape
    R.compare_exact(name + " gx, non-contiguous x", gb[..., 3:W + 3], want_gx)
    assert bool((gb[..., :3] == 0).all()) and bool((gb[..., W + 3:] == 0).all())


@pytest.mark.parametrize("shape,dt", CHAIN_ROWS)
def test_chain_gaussian(shape, dt):
    """Forward: every p within the largest gaussian_bound of stem_fwd's Out over the taps of its window, measured from the
    reference maximum (the maximum is 1-Lipschitz in the sup norm).  Backward: gy restated exactly from the function's saved
    p and idx (no element off the premise), gx within stem_bwd's bound."""
    B, H, W = shape
    OH, OW = H // 2, W // 2
    PH, PW = P.pooled(OH), P.pooled(OW)
    name = f"chain {B}x{H}x{W} {dt} [gaussian]"
    o = _stem_operands("stem_fwd", B, H, W, dt, "gaussian")
    fo = _forward_reference(o)
    r = fo.pre.clamp_min(0)
    want_max, _ = P.maxpool_fwd(r)
    bound, _ = P.maxpool_fwd(R.gaussian_bound(fo, r))
    x = o["x"].clone().requires_grad_(True)
    out = _chain(o, x)
    _check_layout(out, B, PH, PW)
    ratio = float(((out.detach().permute(0, 2, 3, 1).double() - want_max).abs() / bound).max())
    print(f"{name}: forward max |p - max r| / bound = {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)
    saved_p, saved_idx = out.grad_fn.saved_tensors[:2]
    assert torch.equal(R.bits(saved_p), R.bits(out.detach().permute(0, 2, 3, 1)))
    gn = torch.randn((B, PH, PW, 64), generator=P.rng(name, "g")).to(BF16).to(DEV)
    gyr = P.pool_bwd(gn, saved_idx, saved_p, o["scale"], OH, OW)
    assert bool(gyr.exact_sum.all()), f"{name}: {int((~gyr.exact_sum).sum())} elements off the exact-sum premise: another seed"
    bo = R.stem_bwd(R.Arith(), gyr.want, o["w"], o["inv_std"], H, W, dt)["gx"]
    (gx,) = torch.autograd.grad(out, x, gn.permute(0, 3, 1, 2))
    assert gx.dtype == dt and gx.shape == x.shape
    q = R.gaussian_ratio(gx, bo)
    print(f"{name}: backward max |gx - r| / bound = {q:.3f}")
    assert q <= 1.0, (name, q)


def test_fused_stem_module_equals_the_function_bitwise():
    """zoo._FusedStem from a random conv1 / bn1 (negative gammas included) equals ops.resnet_stem on the same packed weights
    with scale / shift of zoo._bn_affine and mean / 1 / std, forward and gradient: pins the module to _init_norm_affine."""
    from dl_attack_on_imagenet_amd import zoo
    gen = torch.Generator().manual_seed(5)
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    bn = torch.nn.BatchNorm2d(64).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(64, 3, 7, 7, generator=gen) * 0.05)
        bn.weight.copy_((0.5 + torch.rand(64, generator=gen)) * (torch.randint(0, 2, (64,), generator=gen) * 2 - 1))
        bn.bias.copy_(0.2 * torch.randn(64, generator=gen))
        bn.running_mean.copy_(0.2 * torch.randn(64, generator=gen))
        bn.running_var.copy_(0.6 + 0.8 * torch.rand(64, generator=gen))
    assert bool((bn.weight < 0).any())
    m = zoo._FusedStem(conv, bn, MEAN, STD).to(DEV)
    scale, shift = (t.to(DEV) for t in zoo._bn_affine(bn))
    assert m.scale.dtype == F32 and torch.equal(m.scale, scale) and torch.equal(m.shift, shift) and bool((scale < 0).any())
    B, H, W = 2, 20, 36
    x0 = torch.rand(B, 3, H, W, generator=gen).to(DEV)
    g = torch.randn(B, P.pooled(H // 2), P.pooled(W // 2), 64, generator=gen).to(BF16).to(DEV).permute(0, 3, 1, 2)
    x1, x2 = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    a = m(x1)
    b = ops().resnet_stem(x2, m.w_fwd, m.w_bwd, scale, shift, MEAN, [1.0 / s for s in STD])
    assert a.dtype == BF16 and a.shape == b.shape and torch.equal(R.bits(a.detach()), R.bits(b.detach()))
    (ga,) = torch.autograd.grad(a, x1, g)
    (gb,) = torch.autograd.grad(b, x2, g)
    assert ga.dtype == F32 and torch.equal(ga.view(torch.int32), gb.view(torch.int32)) and bool(ga.abs().sum() > 0)
