"""MobileNetV2 with all four own_* switches as ONE straight-line sequence of C-ABI calls: forward from the image to the fp32
logits, and the gradient of a given fp32 logit gradient back to the image, with no autograd and no nn.Module.  Written from
the contracts of include/adil_hip.h; every step is one of

    first_fwd  first_bwd  dw_fwd  dw_bwd  pw8_fwd  pw8_bwd  head_fwd  head_bwd

with the arguments of the C ABI under the names the four reference modules give them (first_conv_reference,
depthwise_reference, pointwise8_reference, head_reference).  Two backends run the very same tape code:

Abi      each step is one call of the loaded library through ctypes on contiguous device tensors, with the packings and
         tables of the product (ops.pack_first3x3_weights, wt2d = w2d.t().contiguous(), the fp32 head weight and its
         transpose);
Restate  each step is the restatement of that name over an `Arith`, followed by its `finish`.  Over `Unrounded` the tape
         is a plain fp64 function, which tests/test_mobilenet_wiring_cpu.py holds to the torch modules.

The one thing the product leaves to autograd is the gradient sum at the ten residual joins: the block input receives the
incoming gradient itself (the projection's `res`) and the expansion layer's gx.  The tape adds the two in the storage type
with `add`: two summands, one rounding, no order to get wrong.

Activations are NHWC tensors [B][H][W][C]; pointwise steps see them as rows [B*H*W][C], the head as [B][H*W][C]; the
image and its gradient are NCHW.  `mut` names ONE deliberate wiring mistake (a (name, block index) pair; blocks are the 17
inverted residual blocks, features[1 + index]); the tests assert that each of them is noticed.  Where the mistake named is
not shape-legal in this architecture (an expansion and a projection never have the same width), the mutant uses the
nearest legal reading, said at its line."""
from typing import NamedTuple, Optional

import torch

import classifier_reference as R
import depthwise_reference as DR
import first_conv_reference as FR
import head_reference as HR
import pointwise8_reference as PR
from classifier_reference import BF16, F32, F64

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]             # what zoo.build_classifier puts in front
SHAPES = [(3, 3, 72, 40), (1, 3, 33, 17)]    # grids 36x20, 18x10, 9x5, 5x3, 3x2 (M = 2160 .. 18) and 17x9, 9x5, 5x3, 3x2, 2x1
CLASSES = 10
RES_BLOCKS = [2, 4, 5, 7, 8, 9, 11, 12, 14, 15]                      # the ten blocks with use_res
S2_BLOCKS = [1, 3, 6, 13]
STEPS = ("first_fwd", "first_bwd", "dw_fwd", "dw_bwd", "pw8_fwd", "pw8_bwd", "head_fwd", "head_bwd")


# ------------------------------------------------------------------------------------------------------------- tables
def bn_scale64(bn):
    return bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)


def bn_affine64(bn):
    """Eval-mode BatchNorm as y = x * scale + shift, in fp64 and unrounded."""
    scale = bn_scale64(bn)
    return scale, bn.bias.detach().double() - bn.running_mean.double() * scale


def layer_tables(net, product=False, device="cpu"):
    """The per-layer operands of a plain zoo.MobileNetV2.
    product False: fp64 and unrounded (the proof): weights, (scale, shift) of `bn_affine64`, the depthwise weight times the
      scale as [9][C] with the same shift as its bias, mean and 1 / std of `zoo.Normalize` (whose buffers are fp32).
    product True: the recipe of the product: bf16 weights, `zoo._bn_affine`, `ops.pack_dw3x3_weights` with the fp64 scale and
      the `_OwnDepthwise` bias, the fp32 head, mean and 1 / std as `_init_norm_affine` forms them."""
    from dl_attack_on_imagenet_amd import ops, zoo
    dev = lambda t: t.detach().to(device).contiguous()
    wdt = BF16 if product else F64

    def pw(conv, bn):
        s, b = zoo._bn_affine(bn) if product else bn_affine64(bn)
        return dict(w=dev(conv.weight.detach().reshape(conv.out_channels, conv.in_channels).to(wdt)), scale=dev(s), shift=dev(b))

    def dw(conv, bn):
        s64 = bn_scale64(bn)
        b64 = bn.bias.detach().double() - bn.running_mean.double() * s64
        if product:
            w9c, bias = ops.pack_dw3x3_weights(conv.weight, s64), b64.float()
        else:
            w9c, bias = (conv.weight.detach().double().reshape(-1, 9) * s64[:, None]).t(), b64
        return dict(w9c=dev(w9c), bias=dev(bias), stride=conv.stride[0])

    feats = list(net.features)
    s0, b0 = zoo._bn_affine(feats[0][1]) if product else bn_affine64(feats[0][1])
    if product:
        mean, inv_std = [float(m) for m in MEAN], [1.0 / float(s) for s in STD]
    else:
        f32 = lambda v: float(torch.tensor(v, dtype=F32))
        mean, inv_std = [f32(m) for m in MEAN], [1.0 / f32(s) for s in STD]
    t = dict(mean=tuple(mean), inv_std=tuple(inv_std), blocks=[],
             first=dict(w=dev(feats[0][0].weight.detach().to(wdt)), scale=dev(s0), shift=dev(b0)))
    for blk in feats[1:-1]:
        layers = list(blk.conv)
        t["blocks"].append(dict(expand=pw(layers[0][0], layers[0][1]) if len(layers) == 4 else None,
                                dw=dw(layers[-3][0], layers[-3][1]), proj=pw(layers[-2], layers[-1]), use_res=blk.use_res))
    t["last"] = pw(feats[-1][0], feats[-1][1])
    fc = net.classifier[-1]
    hdt = F32 if product else F64
    t["head"] = dict(w=dev(fc.weight.detach().to(hdt)), bias=dev(fc.bias.detach().to(hdt)))
    return t


# ------------------------------------------------------------------------------------------------------------ backends
def restate(ar, name, **k):
    """The restatement of one step over `ar`: a dict of the reference modules' result objects (FCOut / DwOut / P8Out), or,
    for the head (whose module has no such object), of finished tensors."""
    if name == "first_fwd":
        return dict(y=FR.first_fwd(ar, k["x"], k["w"], k["mean"], k["inv_std"], k["scale"], k["shift"], k["relu6"]))
    if name == "first_bwd":
        return dict(gx=FR.first_bwd(ar, k["g"], k["y"], k["scale"], k["w"], k["inv_std"], k["H"], k["W"], k["relu6"], k["out_dtype"]))
    if name == "dw_fwd":
        return dict(y=DR.dw_fwd(ar, k["x"], k["w9c"], k["bias"], k["stride"], k["relu6"]))
    if name == "dw_bwd":
        return dict(gx=DR.dw_bwd(ar, k["g"], k["y"], k["w9c"], k["H"], k["W"], k["stride"], k["relu6"]))
    if name == "pw8_fwd":
        return dict(y=PR.pw8_fwd(ar, k["x"], k["w"], k["scale"], k["shift"], k["res"], k["act"]))
    if name == "pw8_bwd":
        return dict(gx=PR.pw8_bwd(ar, k["g"], k["y"], k["scale"], k["wt"], k["act"]))
    if name == "head_fwd":
        S, _ = HR.pool_sum(ar, k["x"])
        pooled = HR.pooled_of(ar, S, k["x"].shape[1])
        acc, _ = HR.logits_of(ar, pooled, k["w"], k["bias"])
        return dict(logits=ar.f32(acc), pooled=pooled)
    if name == "head_bwd":
        acc, _ = HR.gpooled_of(ar, k["g"], k["w"])
        gp = ar.f32(acc)
        return dict(gx=HR.gx_of(ar, gp, k["HW"]).to(ar.dtype), gpooled=gp)
    raise KeyError(name)


_FINISH = {"first": FR.finish, "dw": DR.finish, "pw8": PR.finish}


class Restate:
    """Each step: the restatement over `ar`, then the `finish` of its module."""

    def __init__(self, ar):
        self.ar, self.steps = ar, 0

    def step(self, name, **kw):
        self.steps += 1
        out = restate(self.ar, name, **kw)
        fin = _FINISH.get(name.split("_")[0])
        return out if fin is None else {key: fin(self.ar, o) for key, o in out.items()}

    def wt(self, w):
        return w.t()

    def add(self, a, b):
        return self.ar.rnd(a + b)


def _ptr(t):
    import ctypes
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


class Abi:
    """Each step: one call of the loaded library.  `log` keeps (name, arguments, outputs) of every step."""

    def __init__(self, lib, keep_log=False):
        self.lib, self.log, self.keep_log, self._packs = lib, [], keep_log, {}

    def add(self, a, b):
        return torch.add(a, b)

    def _packed(self, w, tag, how):
        key = (w.data_ptr(), tag)
        if key not in self._packs:
            self._packs[key] = (w, how(w))                             # keeps w alive: the pointer stays a valid key
        return self._packs[key][1]

    def wt(self, w):
        return self._packed(w, "t", lambda v: v.t().contiguous())

    def step(self, name, **kw):
        import ctypes
        from dl_attack_on_imagenet_amd import ops
        L, k = self.lib, kw
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        fp32 = ("scale", "shift", "w9c", "bias") + (("x",) if name == "first_fwd" and k["x"].dtype == F32 else ()) \
            + (("g", "w") if name.startswith("head") else ())
        for key, v in k.items():
            if isinstance(v, torch.Tensor):
                assert v.is_cuda and v.is_contiguous(), (name, key)
                assert v.dtype == (F32 if key in fp32 else BF16), (name, key, v.dtype)
        dev = next(v for v in k.values() if isinstance(v, torch.Tensor)).device
        new = lambda *shape, dtype=BF16: torch.empty(shape, dtype=dtype, device=dev)
        code = lambda dtype: {F32: 0, BF16: 1}[dtype]
        if name == "first_fwd":
            B, C, H, W = k["x"].shape
            assert C == 3 and k["w"].shape == (32, 3, 3, 3)
            OH, OW = FR.out_grid(H, W)
            out = dict(y=new(B, OH, OW, 32))
            w_fwd = self._packed(k["w"], "first", ops.pack_first3x3_weights)[0]
            rc = L.adil_first3x3_fwd(_ptr(k["x"]), code(k["x"].dtype), _ptr(w_fwd), *k["mean"], *k["inv_std"], _ptr(k["scale"]),
                                     _ptr(k["shift"]), _ptr(out["y"]), B, H, W, int(k["relu6"]), st)
        elif name == "first_bwd":
            (B, OH, OW, N), H, W = k["g"].shape, k["H"], k["W"]
            assert N == 32 and (OH, OW) == FR.out_grid(H, W) and (k["y"] is None or k["y"].shape == k["g"].shape)
            out = dict(gx=new(B, 3, H, W, dtype=k["out_dtype"]))
            w_bwd = self._packed(k["w"], "first", ops.pack_first3x3_weights)[1]
            rc = L.adil_first3x3_bwd(_ptr(k["g"]), _ptr(k["y"]), _ptr(k["scale"]), _ptr(w_bwd), *k["inv_std"], _ptr(out["gx"]),
                                     code(k["out_dtype"]), B, H, W, int(k["relu6"]), st)
        elif name == "dw_fwd":
            (B, H, W, C), s = k["x"].shape, k["stride"]
            assert k["w9c"].shape == (9, C) and k["bias"].shape == (C,) and s in (1, 2)
            out = dict(y=new(B, DR.out_size(H, s), DR.out_size(W, s), C))
            rc = L.adil_dw3x3_fwd(_ptr(k["x"]), _ptr(k["w9c"]), _ptr(k["bias"]), _ptr(out["y"]), B, H, W, C, s, int(k["relu6"]), st)
        elif name == "dw_bwd":
            (B, OH, OW, C), H, W, s = k["g"].shape, k["H"], k["W"], k["stride"]
            assert (OH, OW) == (DR.out_size(H, s), DR.out_size(W, s)) and k["w9c"].shape == (9, C)
            assert k["y"] is None or k["y"].shape == k["g"].shape
            out = dict(gx=new(B, H, W, C))
            rc = L.adil_dw3x3_bwd(_ptr(k["g"]), _ptr(k["y"]), _ptr(k["w9c"]), _ptr(out["gx"]), B, H, W, C, s, int(k["relu6"]), st)
        elif name == "pw8_fwd":
            (M, K), N = k["x"].shape, k["w"].shape[0]
            assert k["w"].shape == (N, K) and k["scale"].shape == (N,) and k["shift"].shape == (N,)
            assert k["res"] is None or (k["res"].shape == (M, N) and not k["act"])
            out = dict(y=new(M, N))
            rc = L.adil_pw8_fwd(_ptr(k["x"]), _ptr(k["w"]), _ptr(k["scale"]), _ptr(k["shift"]), _ptr(k["res"]), _ptr(out["y"]), M, K, N,
                                int(k["act"]), st)
        elif name == "pw8_bwd":
            (M, N), K = k["g"].shape, k["wt"].shape[0]
            assert k["wt"].shape == (K, N) and k["scale"].shape == (N,) and (k["y"] is None or k["y"].shape == (M, N))
            assert (k["y"] is not None) == bool(k["act"])
            out = dict(gx=new(M, K))
            rc = L.adil_pw8_bwd(_ptr(k["g"]), _ptr(k["y"]), _ptr(k["scale"]), _ptr(k["wt"]), _ptr(out["gx"]), M, K, N, int(k["act"]), st)
        elif name == "head_fwd":
            (B, HW, C), N = k["x"].shape, k["w"].shape[0]
            assert k["w"].shape == (N, C) and k["bias"].shape == (N,)
            out = dict(logits=new(B, N, dtype=F32), pooled=new(B, C, dtype=F32))
            rc = L.adil_pool_head_fwd(_ptr(k["x"]), _ptr(self.wt(k["w"])), _ptr(k["bias"]), _ptr(out["pooled"]), _ptr(out["logits"]),
                                      B, HW, C, N, st)
        elif name == "head_bwd":
            (B, N), C, HW = k["g"].shape, k["w"].shape[1], k["HW"]
            assert k["w"].shape == (N, C)
            out = dict(gx=new(B, HW, C), gpooled=new(B, C, dtype=F32))
            rc = L.adil_pool_head_bwd(_ptr(k["g"]), _ptr(k["w"]), _ptr(out["gpooled"]), _ptr(out["gx"]), B, HW, C, N, st)
        else:
            raise KeyError(name)
        assert rc == 0, (name, rc)
        if self.keep_log:
            self.log.append((name, kw, out))
        return out


def step_ratios(log):
    """Every logged step of an `Abi` tape against its fp64 restatement on the step's actual inputs: the worst
    max |err| / bound per step name, the bounds being the derived element-wise ones of the four reference modules.  The
    head's gx is a bit-defined function of the stored gpooled and is compared bit for bit (head_reference.gaussian_ratios)."""
    ar, worst, count = R.Arith(), {}, {}
    ratio = {"first": FR.gaussian_ratio, "dw": DR.gaussian_ratio, "pw8": PR.gaussian_ratio}
    note = lambda name, q: (worst.__setitem__(name, max(worst.get(name, 0.0), q)), count.__setitem__(name, count.get(name, 0) + 1))
    head = {}
    for name, kw, out in log:
        if name.startswith("head"):
            head[name] = (kw, out)
            continue
        ref = restate(ar, name, **kw)
        for key, got in out.items():
            q = ratio[name.split("_")[0]](got, ref[key])
            note(name, q if q == q else float("inf"))
    if head:
        c = lambda t: t.detach().cpu()
        (kf, of), (kb, ob) = head["head_fwd"], head["head_bwd"]
        op = HR.Operands(c(kf["x"]), c(kf["w"]), c(kf["bias"]), c(kb["g"]), None)
        got = HR.Results(c(of["pooled"]), c(of["logits"]), c(ob["gpooled"]), c(ob["gx"]))
        rp, rl, rg = HR.gaussian_ratios("tape head", op, got)
        note("head_fwd", max(rp, rl))
        note("head_bwd", rg)
    return worst, count


# ---------------------------------------------------------------------------------------------------------------- tape
class Tape(NamedTuple):
    outs: list                       # the 19 outputs of features[0 .. 18], NHWC
    logits: torch.Tensor             # [B][classes], fp32 on the rounded backends
    pooled: torch.Tensor             # [B][1280]
    grad: Optional[torch.Tensor]     # gradient with respect to the image, NCHW, in the image's dtype on the rounded backends
    acts: list                       # the 35 ReLU6 outputs in network order (first conv, expansions and depthwise layers, last 1x1)


def _rows(t):
    return None if t is None else t.reshape(-1, t.shape[-1])


def _up2(g, H, W):
    out = torch.zeros(g.shape[0], H, W, g.shape[3], dtype=g.dtype, device=g.device)
    out[:, ::2, ::2] = g
    return out


def run_tape(be, tables, x, g_logits, mut=None):
    """x: the image [B][3][H][W], fp32 or bf16 (contiguous NCHW); g_logits: fp32 [B][classes] or None (forward only)."""
    mname, mblock = mut if mut is not None else (None, -1)
    hit = lambda name, i: mname == name and mblock == i
    T, step = tables, be.step
    B, _, H, W = x.shape
    f = T["first"]
    y0 = step("first_fwd", x=x, w=f["w"], mean=T["mean"], inv_std=T["inv_std"], scale=f["scale"], shift=f["shift"], relu6=1)["y"]
    outs, acts, saved, h = [y0], [y0], [], y0
    # ------------------------------------------------------------------------------------------------------ forward
    for i, t in enumerate(T["blocks"]):
        xin, e, d, p = h, t["expand"], t["dw"], t["proj"]
        b, hh, ww, _ = xin.shape
        he = xin
        if e is not None:
            he = step("pw8_fwd", x=_rows(xin), w=e["w"], scale=e["scale"], shift=e["shift"], res=None, act=1)["y"].reshape(b, hh, ww, -1)
            acts.append(he)
        hd = step("dw_fwd", x=he, w9c=d["w9c"], bias=d["bias"], stride=d["stride"], relu6=1)["y"]
        acts.append(hd)
        res = xin if t["use_res"] else None
        if hit("drop_res_fwd", i):                                     # mutant: a residual block without its residual
            assert t["use_res"]
            res = None
        if hit("res_on_plain", i):                                     # mutant: a non-residual block given `res`; no such block
            n = p["w"].shape[0]                                        # has input and output of one shape: the input's first
            assert not t["use_res"] and d["stride"] == 1 and xin.shape[3] >= n     # channels stand in for it
            res = xin[..., :n].contiguous()
        out = step("pw8_fwd", x=_rows(hd), w=p["w"], scale=p["scale"], shift=p["shift"], res=_rows(res), act=0)["y"]
        out = out.reshape(hd.shape[:3] + (-1,))
        saved.append((xin, he, hd, out))
        outs.append(out)
        h = out
    l = T["last"]
    b, hh, ww, _ = h.shape
    hl = step("pw8_fwd", x=_rows(h), w=l["w"], scale=l["scale"], shift=l["shift"], res=None, act=1)["y"].reshape(b, hh, ww, -1)
    outs.append(hl)
    acts.append(hl)
    hd_ = T["head"]
    o = step("head_fwd", x=hl.reshape(b, hh * ww, -1), w=hd_["w"], bias=hd_["bias"])
    logits, pooled = o["logits"], o["pooled"]
    if g_logits is None:
        return Tape(outs, logits, pooled, None, acts)
    # ----------------------------------------------------------------------------------------------------- backward
    g = step("head_bwd", g=g_logits, w=hd_["w"], HW=hh * ww)["gx"]
    g = step("pw8_bwd", g=_rows(g), y=_rows(hl), scale=l["scale"], wt=be.wt(l["w"]), act=1)["gx"].reshape(h.shape)
    for i in range(len(saved) - 1, -1, -1):
        t = T["blocks"][i]
        xin, he, hd, out = saved[i]
        e, d, p = t["expand"], t["dw"], t["proj"]
        g_out = g
        ps, es = p["scale"], (None if e is None else e["scale"])
        if hit("swap_scale_bwd", i):                                   # mutant: the two layers' scale tables swapped in the
            n, k = ps.shape[0], es.shape[0]                            # backward; their widths differ by the expansion factor:
            ps, es = es[:n].contiguous(), ps.repeat(k // n)            # the expansion's first entries / the projection's repeated
        g_hd = step("pw8_bwd", g=_rows(g_out), y=None, scale=ps, wt=be.wt(p["w"]), act=0)["gx"].reshape(hd.shape)
        bh, hh, ww, _ = he.shape
        if hit("dw_no_mask", i):                                       # mutant: the depthwise gradient without its ReLU6 mask
            g_he = step("dw_bwd", g=g_hd, y=None, w9c=d["w9c"], H=hh, W=ww, stride=d["stride"], relu6=0)["gx"]
        elif hit("s2_as_s1", i):                                       # mutant: a stride-2 gradient scattered as stride 1 on
            assert d["stride"] == 2                                    # the output grid, then placed on the sub-grid
            sub = step("dw_bwd", g=g_hd, y=hd, w9c=d["w9c"], H=hd.shape[1], W=hd.shape[2], stride=1, relu6=1)["gx"]
            g_he = _up2(sub, hh, ww)
        else:
            g_he = step("dw_bwd", g=g_hd, y=hd, w9c=d["w9c"], H=hh, W=ww, stride=d["stride"], relu6=1)["gx"]
        if e is not None:
            y = he
            if hit("expand_mask_from_proj", i):                        # mutant: the expansion's mask from the projection's
                assert t["use_res"]                                    # output, its channels repeated to the expansion's width
                y = out.repeat(1, 1, 1, he.shape[3] // out.shape[3])
            g_x = step("pw8_bwd", g=_rows(g_he), y=_rows(y), scale=es, wt=be.wt(e["w"]), act=1)["gx"].reshape(xin.shape)
        else:
            g_x = g_he
        if t["use_res"] and not (hit("drop_res_grad", i) or mname == "drop_res_grad_all"):
            g = be.add(g_out, g_x)                                     # autograd's sum at the join
        else:
            g = g_x                                                    # (mutants: the residual gradient dropped here / everywhere)
    gx = step("first_bwd", g=g, y=y0, scale=f["scale"], w=f["w"], inv_std=T["inv_std"], H=H, W=W, relu6=1,
              out_dtype=BF16 if x.dtype == BF16 else F32)["gx"]
    return Tape(outs, logits, pooled, gx, acts)


def relu6_shares(tape):
    """(share at 0, share strictly inside (0, 6), share at 6) of each of the 35 ReLU6 outputs."""
    out = []
    for a in tape.acts:
        n = a.numel()
        zero, six = int((a == 0).sum()), int((a == 6).sum())
        out.append((zero / n, (n - zero - six) / n, six / n))
    return out


def assert_premises(tape, name=""):
    """What a run must exercise, asserted on the reference tape before any kernel result is looked at."""
    shares = relu6_shares(tape)
    assert len(shares) == 35 and len(tape.outs) == 19
    for i, (zero, inside, six) in enumerate(shares):
        assert zero > 0 and inside > 0, f"{name}: ReLU6 layer {i} has shares {zero:.4f} / {inside:.4f} / {six:.4f}"
        assert i == 0 or six > 0, f"{name}: ReLU6 layer {i} has no element at 6"
    for i, o in enumerate(tape.outs):
        assert bool(torch.isfinite(o.double()).all()), f"{name}: the output of features[{i}] is not finite"
    if tape.grad is not None:
        for c in range(3):
            assert float(tape.grad[:, c].double().abs().max()) > 0, f"{name}: the image gradient of channel {c} is zero"
    return shares


# ------------------------------------------------------------------------------------------------------------ networks
def make_inputs(shape, seed=3):
    """(x fp32 [B][3][H][W] in [0, 1], g_logits fp32 [B][classes]): structured images of size 72, cropped."""
    from structured import structured_images
    B, _, H, W = shape
    assert H <= 72 and W <= 72
    images, _ = structured_images(B, classes=4, seed=seed, size=72)
    g = torch.randn(B, CLASSES, generator=torch.Generator().manual_seed(seed + 100))
    return images[:, :, :H, :W].contiguous(), g.contiguous()


def make_net(seed=5):
    """A zoo.MobileNetV2 (fp32, eval, frozen, 10 classes): seeded weights, the convolution weights rounded to bf16, every
    BatchNorm randomised by the "images given" recipe of tests/test_gpu_pointwise8.py::randomised_checkpoint on the images
    of SHAPES[0]: one training-mode pass with momentum 1, the statistics then perturbed channel by channel, gamma of both
    signs, beta 0.3 N(0,1).  (On the "around 0 / 1" recipe the input gradient of this architecture is about 1e-9.)"""
    from dl_attack_on_imagenet_amd import zoo
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = zoo.MobileNetV2(num_classes=CLASSES)
    model = torch.nn.Sequential(zoo.Normalize(MEAN, STD), net)
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    gen = torch.Generator().manual_seed(seed + 1)
    r = lambda n: torch.randn(n, generator=gen)
    u = lambda n: torch.rand(n, generator=gen)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(m.weight.bfloat16().float())
        for m in bns:
            m.momentum = 1.0
            m.train()
        net.classifier.eval()
        model(make_inputs(SHAPES[0])[0])
        model.eval()
        for m in bns:
            n = m.num_features
            m.momentum = 0.1
            m.running_mean.mul_(1 + 0.2 * r(n)).add_(0.1 * m.running_var.sqrt() * r(n))
            m.running_var.mul_(0.6 + 0.8 * u(n))
            m.weight.copy_((0.7 + 0.6 * u(n)) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1))
            m.bias.copy_(0.3 * r(n))
    for q in net.parameters():
        q.requires_grad_(False)
    return net.eval()
