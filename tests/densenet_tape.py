"""A zoo.DenseNet of any block_config with all six own_dense_* switches as ONE straight-line sequence of C-ABI calls: forward
from the image to the fp32 logits, and the gradient of a given fp32 logit gradient back to the image, with no autograd and
no nn.Module.  Written from the contracts of include/adil_hip.h; every step is one of

    stem_fwd  pool_fwd  pool_bwd  stem_bwd  d1_fwd  d1_bwd  d3_fwd  d3_bwd  tr_fwd  tr_bwd  head_fwd  head_bwd

with the arguments of the C ABI under the names the reference modules give them (classifier_reference.stem_fwd / stem_bwd,
stem_pool_reference, dense1x1_reference, dense3x3_reference = classifier_reference.conv3x3 / conv3x3_bwd,
dense_block_reference.accumulate, dense_transition_reference, dense_head_reference).  Two backends run the very same tape
code:

Abi      each step is one call of the loaded library through ctypes on contiguous device tensors, with the packings of the
         product (ops.pack_stem_weights, ops.pack_conv3x3_weights, wt = w.t().contiguous(), the fp32 head weight and its
         transpose);
Restate  each step is the restatement of that name over an `Arith`, followed by its module's `finish`.  Over `Unrounded`
         the tape is a plain fp64 function, which tests/test_densenet_wiring_cpu.py holds to the torch modules.

The tape does not share the product's addressing.  The product keeps a dense block in ONE buffer [M][Ctot] and hands the
kernels channel offsets and the pitch Ctot; here a block is a Python LIST of contiguous tensors, the block input [M][C0]
and one [M][growth] tensor per layer.  Layer i reads the contiguous concatenation of the first i + 1 of them through the
plain entry point and appends its output.  Backwards the gradient is a list of the same shapes: layer i takes the
gradient of its own output from the list, and the gradient of the features it read, concatenated to a contiguous
[M][off_i] tensor, is the `old` operand of adil_dense1x1_bwd_ld with ldgx = off_i and accumulate = 1; what comes back
replaces those list entries.  The layers are walked LAST LAYER FIRST and every contribution is one fp32 add followed by
one rounding: the specification in `ops.DenseBlockFunction`'s docstring, which the `Restate` backend realises with
dense_block_reference.accumulate.  A transition receives the gradient list's first entry, a contiguous tensor (the product
reads it in place at pitch Ctot).

Activations are NHWC tensors [B][H][W][C]; 1x1 steps see them as rows [B*H*W][C], the head as [B][H*W][C]; the image and
its gradient are NCHW.  `mut` names ONE deliberate wiring mistake as (name, block or transition index, layer index); the
tests assert that each of them is noticed.  Every mutant keeps all shapes legal; where the mistake named is not
shape-legal as it stands, the nearest legal reading is used and said at its line."""
from typing import NamedTuple, Optional

import torch

import classifier_reference as R
import dense1x1_reference as D1
import dense_block_reference as DB
import dense_head_reference as DH
import dense_transition_reference as DT
import head_reference as HR
import stem_pool_reference as SP
from classifier_reference import BF16, F32, F64

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]             # what zoo.build_classifier puts in front
# conv grids 48x16 / 47x31 (odd: the max-pool's last window is partial); block grids 24x8, 12x4, 6x2, 3x1 (M = 384, 96,
# 24, 6) and 24x16, 12x8, 6x4, 3x2 (M = 384, 96, 24, 6)
SHAPES = [(2, 3, 96, 32), (1, 3, 94, 62)]
CLASSES = 10
REDUCED, REAL = (3, 4, 2, 2), (6, 12, 24, 16)
STEPS = ("stem_fwd", "pool_fwd", "pool_bwd", "stem_bwd", "d1_fwd", "d1_bwd", "d3_fwd", "d3_bwd", "tr_fwd", "tr_bwd", "head_fwd",
         "head_bwd")
SHARE = (0.05, 0.95)             # every ReLU of the network keeps a share of its elements inside this interval


def point_names(n_blocks=4):
    """The eight points of a four-block network in forward order: the pooled stem output, then block and transition outputs."""
    out = ["stem output"]
    for b in range(n_blocks):
        out.append("output of denseblock%d" % (b + 1))
        if b != n_blocks - 1:
            out.append("output of transition%d" % (b + 1))
    return out


def step_counts(block_config):
    """How many steps of each name one forward + backward tape of a network makes."""
    n, t = sum(block_config), len(block_config) - 1
    return {"stem_fwd": 1, "pool_fwd": 1, "pool_bwd": 1, "stem_bwd": 1, "d1_fwd": n, "d1_bwd": n, "d3_fwd": n, "d3_bwd": n,
            "tr_fwd": t, "tr_bwd": t, "head_fwd": 1, "head_bwd": 1}


# ------------------------------------------------------------------------------------------------------------- tables
def bn_affine64(bn):
    """Eval-mode BatchNorm as y = x * scale + shift, in fp64 and unrounded."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.double() * scale


def layer_tables(net, product=False, device="cpu"):
    """The operands of a plain zoo.DenseNet, block by block.
    product False: fp64 and unrounded (the proof): weights, (scale, shift) of `bn_affine64`, mean and 1 / std of
      `zoo.Normalize` (whose buffers are fp32).
    product True: the recipe of the product: bf16 weights, `zoo._bn_affine`, the transposed 1x1 weights, the two layouts of
      `ops.pack_conv3x3_weights` and of `ops.pack_stem_weights`, the fp32 head with its transpose, mean and 1 / std as
      `zoo._init_norm_affine` forms them."""
    from dl_attack_on_imagenet_amd import ops, zoo
    dev = lambda t: t.detach().to(device).contiguous()
    wdt = BF16 if product else F64
    affine = zoo._bn_affine if product else bn_affine64

    def one_by_one(pre_bn, conv, bn):
        ps, pb = affine(pre_bn)
        w = conv.weight.detach().reshape(conv.out_channels, conv.in_channels).to(wdt)
        t = dict(pscale=dev(ps), pshift=dev(pb), w=dev(w))
        if bn is not None:
            s, b = affine(bn)
            t.update(scale=dev(s), shift=dev(b))
        if product:
            t["wt"] = dev(w.t())
        return t

    f = net.features
    s0, b0 = affine(f.norm0)
    stem = dict(w=dev(f.conv0.weight.detach().to(wdt)), scale=dev(s0), shift=dev(b0))
    if product:
        stem["w_fwd"], stem["w_bwd"] = (dev(t) for t in ops.pack_stem_weights(f.conv0.weight.detach().to(wdt)))
        mean, inv_std = [float(m) for m in MEAN], [1.0 / float(s) for s in STD]
    else:
        f32 = lambda v: float(torch.tensor(v, dtype=F32))
        mean, inv_std = [f32(m) for m in MEAN], [1.0 / f32(s) for s in STD]
    T = dict(mean=tuple(mean), inv_std=tuple(inv_std), stem=stem, blocks=[], trans=[])
    for name, m in f.named_children():
        if name.startswith("denseblock"):
            layers = []
            for layer in m.values():
                t = one_by_one(layer.norm1, layer.conv1, layer.norm2)
                t["w3"] = dev(layer.conv2.weight.detach().to(wdt))
                if product:
                    t["wp_fwd"], t["wp_bwd"] = (dev(p) for p in ops.pack_conv3x3_weights(layer.conv2.weight.detach().to(wdt)))
                layers.append(t)
            T["blocks"].append(layers)
        elif name.startswith("transition"):
            T["trans"].append(one_by_one(m.norm, m.conv, None))
    ps, pb = affine(f.norm5)
    hdt = F32 if product else F64
    w = net.classifier.weight.detach().to(hdt)
    T["head"] = dict(pscale=dev(ps), pshift=dev(pb), w=dev(w), bias=dev(net.classifier.bias.detach().to(hdt)))
    if product:
        T["head"]["wt"] = dev(w.t())
    return T


# ------------------------------------------------------------------------------------------------------------ backends
def _rows(t):
    return None if t is None else t.reshape(-1, t.shape[-1])


def restate(ar, name, **k):
    """The restatement of one step over `ar`: a dict of finished tensors (values, in the arithmetic's dtype), and under the
    keys that start with "_" the reference modules' result objects, for the bounds of `step_ratios`."""
    if name == "stem_fwd":
        o = R.stem_fwd(ar, k["x"], k["w"], k["mean"], k["inv_std"], k["scale"], k["shift"])["y"]
        return dict(y=R.finish(ar, o), _y=o)
    if name == "stem_bwd":
        o = R.stem_bwd(ar, k["gy"], k["w"], k["inv_std"], k["H"], k["W"], k["out_dtype"])["gx"]
        return dict(gx=R.finish(ar, o), _gx=o)
    if name == "pool_fwd":
        p, idx = SP.maxpool_fwd(k["y"])
        return dict(p=p.to(ar.dtype), idx=idx)
    if name == "pool_bwd":
        ref = SP.pool_bwd(k["g"], k["idx"], k["p"], k["scale"], k["OH"], k["OW"])
        return dict(gy=SP.gy_of(ar, ref).to(ar.dtype), _gy=ref)
    if name == "d1_fwd":
        o = D1.d1_fwd(ar, k["x"], k["pscale"], k["pshift"], k["w"], k["scale"], k["shift"], k["act"])
        return dict(y=D1.finish(ar, o), _y=o)
    if name == "d1_bwd":
        o = D1.d1_bwd(ar, k["g"], k["y"], k["scale"], k["wt"], k["xin"], k["pscale"], k["pshift"], k["act"])
        if k["accumulate"]:
            o = DB.accumulate(ar, o, k["old"])
        return dict(gx=D1.finish(ar, o), _gx=o)
    if name == "d3_fwd":
        o = R.conv3x3(ar, k["x"], k["w"])["y"]
        return dict(y=R.finish(ar, o), _y=o)
    if name == "d3_bwd":
        o = R.conv3x3_bwd(ar, k["g"], k["w"])["gx"]
        return dict(gx=R.finish(ar, o), _gx=o)
    if name == "tr_fwd":
        B, H, W, K = k["x"].shape
        o = DT.tr_fwd(ar, (B, H, W, K, k["w"].shape[0]), _rows(k["x"]), k["pscale"], k["pshift"], k["w"])
        return dict(y=D1.finish(ar, o).reshape(B, H // 2, W // 2, -1), _y=o)
    if name == "tr_bwd":
        B, H, W, K = k["xin"].shape
        o = DT.tr_bwd(ar, (B, H, W, K, k["wt"].shape[1]), _rows(k["g"]), k["wt"], _rows(k["xin"]), k["pscale"], k["pshift"])
        return dict(gx=D1.finish(ar, o).reshape(B, H, W, K), _gx=o)
    if name == "head_fwd":
        pre = DH.pre_of(ar, k["x"], k["pscale"], k["pshift"])
        pooled = DH.pooled_of(ar, DH.post_of(ar, pre), k["x"].shape[1])[0]
        acc, _ = HR.logits_of(ar, pooled, k["w"], k["bias"])
        return dict(logits=ar.f32(acc), pooled=pooled)
    if name == "head_bwd":
        acc, _ = HR.gpooled_of(ar, k["g"], k["w"])
        gp = ar.f32(acc)
        return dict(gx=DH.gx_of(ar, gp, k["x"], k["pscale"], k["pshift"]).to(ar.dtype), gpooled=gp)
    raise KeyError(name)


class Restate:
    """Each step: the restatement over `ar` with its module's `finish`."""

    def __init__(self, ar):
        self.ar, self.steps = ar, 0

    def step(self, name, **kw):
        self.steps += 1
        return {key: v for key, v in restate(self.ar, name, **kw).items() if not key.startswith("_")}

    def wt(self, w, given=None):
        return w.t()

    def affine(self, x, scale, shift):
        """A BatchNorm alone (the mutant `norm5_twice` only): x * scale + shift, rounded to the storage type."""
        ar = self.ar
        return ar.rnd(ar.f32(x) * ar.f32(scale) + ar.f32(shift)).to(ar.dtype)


def _ptr(t):
    import ctypes
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


_DTYPES = {"x": BF16, "y": BF16, "g": BF16, "gy": BF16, "p": BF16, "xin": BF16, "old": BF16, "w": BF16, "wt": BF16,
           "wp_fwd": BF16, "wp_bwd": BF16, "w_fwd": BF16, "w_bwd": BF16, "idx": torch.uint8, "pscale": F32, "pshift": F32,
           "scale": F32, "shift": F32, "bias": F32}


class Abi:
    """Each step: one call of the loaded library on contiguous tensors.  `log` keeps (name, arguments, outputs) of every
    step.  The packed layouts come with the step (the product's tables) or are formed here by the product's packers."""

    def __init__(self, lib, keep_log=False):
        self.lib, self.log, self.keep_log, self._packs = lib, [], keep_log, {}

    def _packed(self, w, tag, how):
        key = (w.data_ptr(), tag)
        if key not in self._packs:
            self._packs[key] = (w, how(w))                             # keeps w alive: the pointer stays a valid key
        return self._packs[key][1]

    def wt(self, w, given=None):
        return given if given is not None else self._packed(w, "t", lambda v: v.t().contiguous())

    def affine(self, x, scale, shift):
        raise NotImplementedError("the mutant norm5_twice runs on the Restate backend only")

    def step(self, name, **kw):
        import ctypes
        from dl_attack_on_imagenet_amd import ops
        L, k = self.lib, kw
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        head = name.startswith("head")
        for key, v in k.items():
            if isinstance(v, torch.Tensor):
                want = _DTYPES[key]
                if (head and key in ("g", "w", "wt")) or (name == "stem_fwd" and key == "x" and v.dtype == F32):
                    want = F32
                assert v.is_cuda and v.is_contiguous() and v.dtype == want, (name, key, v.dtype)
        dev = next(v for v in k.values() if isinstance(v, torch.Tensor)).device
        new = lambda *shape, dtype=BF16: torch.empty(shape, dtype=dtype, device=dev)
        code = lambda dtype: {F32: 0, BF16: 1}[dtype]
        if name == "stem_fwd":
            B, C, H, W = k["x"].shape
            assert C == 3 and k["w"].shape == (64, 3, 7, 7) and H % 2 == 0 and W % 2 == 0
            w_fwd = k.get("w_fwd") if k.get("w_fwd") is not None else self._packed(k["w"], "stem", ops.pack_stem_weights)[0]
            assert w_fwd.shape == (64, 224) and k["scale"].shape == (64,) and k["shift"].shape == (64,)
            out = dict(y=new(B, H // 2, W // 2, 64))
            rc = L.adil_stem_conv_fwd(_ptr(k["x"]), code(k["x"].dtype), _ptr(w_fwd), *k["mean"], *k["inv_std"], _ptr(k["scale"]),
                                      _ptr(k["shift"]), _ptr(out["y"]), B, H, W, st)
        elif name == "pool_fwd":
            B, OH, OW, C = k["y"].shape
            out = dict(p=new(B, SP.pooled(OH), SP.pooled(OW), C), idx=new(B, SP.pooled(OH), SP.pooled(OW), C, dtype=torch.uint8))
            rc = L.adil_maxpool_fwd(_ptr(k["y"]), _ptr(out["p"]), _ptr(out["idx"]), B, OH, OW, C, st)
        elif name == "pool_bwd":
            (B, PH, PW, C), OH, OW = k["g"].shape, k["OH"], k["OW"]
            assert (PH, PW) == (SP.pooled(OH), SP.pooled(OW)) and k["idx"].shape == k["g"].shape == k["p"].shape
            assert k["scale"].shape == (C,)
            out = dict(gy=new(B, OH, OW, C))
            rc = L.adil_stem_pool_bwd(_ptr(k["g"]), _ptr(k["idx"]), _ptr(k["p"]), _ptr(k["scale"]), _ptr(out["gy"]), B, OH, OW, C, st)
        elif name == "stem_bwd":
            (B, OH, OW, C), H, W = k["gy"].shape, k["H"], k["W"]
            assert C == 64 and (OH, OW) == (H // 2, W // 2) and H % 2 == 0 and W % 2 == 0
            w_bwd = k.get("w_bwd") if k.get("w_bwd") is not None else self._packed(k["w"], "stem", ops.pack_stem_weights)[1]
            assert w_bwd.shape == (4, 49 * 64)
            out = dict(gx=new(B, 3, H, W, dtype=k["out_dtype"]))
            rc = L.adil_stem_conv_bwd(_ptr(k["gy"]), _ptr(w_bwd), *k["inv_std"], _ptr(out["gx"]), code(k["out_dtype"]), B, H, W, st)
        elif name == "d1_fwd":
            (M, K), N = k["x"].shape, k["w"].shape[0]
            assert k["w"].shape == (N, K) and k["pscale"].shape == (K,) and k["pshift"].shape == (K,)
            assert k["scale"].shape == (N,) and k["shift"].shape == (N,)
            out = dict(y=new(M, N))
            rc = L.adil_dense1x1_fwd(_ptr(k["x"]), _ptr(k["pscale"]), _ptr(k["pshift"]), _ptr(k["w"]), _ptr(k["scale"]),
                                     _ptr(k["shift"]), _ptr(out["y"]), M, K, N, int(k["act"]), st)
        elif name == "d1_bwd":
            (M, N), K = k["g"].shape, k["wt"].shape[0]
            assert k["wt"].shape == (K, N) and k["xin"].shape == (M, K) and k["scale"].shape == (N,)
            assert k["pscale"].shape == (K,) and k["pshift"].shape == (K,)
            assert (k["y"] is not None) == bool(k["act"]) and (k["y"] is None or k["y"].shape == (M, N))
            if k["accumulate"]:
                assert k["old"].shape == (M, K)
                out = dict(gx=k["old"].clone())                        # the kernel adds in place: the operand stays as it was
            else:
                out = dict(gx=new(M, K))
            rc = L.adil_dense1x1_bwd_ld(_ptr(k["g"]), N, _ptr(k["y"]), N, _ptr(k["scale"]), _ptr(k["wt"]), _ptr(k["xin"]), K,
                                        _ptr(k["pscale"]), _ptr(k["pshift"]), _ptr(out["gx"]), K, int(k["accumulate"]), M, K, N,
                                        int(k["act"]), st)
        elif name == "d3_fwd":
            (B, H, W, C), N = k["x"].shape, k["w"].shape[0]
            assert k["w"].shape == (N, C, 3, 3)
            wp = k.get("wp_fwd") if k.get("wp_fwd") is not None else self._packed(k["w"], "3x3", ops.pack_conv3x3_weights)[0]
            assert wp.shape == (N, 9 * C)
            out = dict(y=new(B, H, W, N))
            rc = L.adil_dense3x3_fwd(_ptr(k["x"]), _ptr(wp), _ptr(out["y"]), B, H, W, C, N, st)
        elif name == "d3_bwd":
            (B, H, W, N), C = k["g"].shape, k["w"].shape[1]
            assert k["w"].shape == (N, C, 3, 3)
            wp = k.get("wp_bwd") if k.get("wp_bwd") is not None else self._packed(k["w"], "3x3", ops.pack_conv3x3_weights)[1]
            assert wp.shape == (C, 9 * N)
            out = dict(gx=new(B, H, W, C))
            rc = L.adil_dense3x3_bwd(_ptr(k["g"]), _ptr(wp), _ptr(out["gx"]), B, H, W, C, N, st)
        elif name == "tr_fwd":
            (B, H, W, K), N = k["x"].shape, k["w"].shape[0]
            assert k["w"].shape == (N, K) and k["pscale"].shape == (K,) and k["pshift"].shape == (K,) and H % 2 == 0 and W % 2 == 0
            out = dict(y=new(B, H // 2, W // 2, N))
            rc = L.adil_dense_transition_fwd(_ptr(k["x"]), _ptr(k["pscale"]), _ptr(k["pshift"]), _ptr(k["w"]), _ptr(out["y"]),
                                             B, H, W, K, N, st)
        elif name == "tr_bwd":
            (B, H, W, K), N = k["xin"].shape, k["wt"].shape[1]
            assert k["wt"].shape == (K, N) and k["g"].shape == (B, H // 2, W // 2, N) and H % 2 == 0 and W % 2 == 0
            assert k["pscale"].shape == (K,) and k["pshift"].shape == (K,)
            out = dict(gx=new(B, H, W, K))
            rc = L.adil_dense_transition_bwd(_ptr(k["g"]), N, _ptr(k["wt"]), _ptr(k["xin"]), _ptr(k["pscale"]), _ptr(k["pshift"]),
                                             _ptr(out["gx"]), B, H, W, K, N, st)
        elif name == "head_fwd":
            (B, HW, C), N = k["x"].shape, k["w"].shape[0]
            assert k["w"].shape == (N, C) and k["bias"].shape == (N,) and k["pscale"].shape == (C,) and k["pshift"].shape == (C,)
            wt = self.wt(k["w"], k.get("wt"))
            assert wt.shape == (C, N)
            out = dict(logits=new(B, N, dtype=F32), pooled=new(B, C, dtype=F32))
            rc = L.adil_bn_pool_head_fwd(_ptr(k["x"]), _ptr(k["pscale"]), _ptr(k["pshift"]), _ptr(wt), _ptr(k["bias"]),
                                         _ptr(out["pooled"]), _ptr(out["logits"]), B, HW, C, N, st)
        elif name == "head_bwd":
            (B, N), (_, HW, C) = k["g"].shape, k["x"].shape
            assert k["w"].shape == (N, C) and k["x"].shape[0] == B and k["pscale"].shape == (C,) and k["pshift"].shape == (C,)
            out = dict(gx=new(B, HW, C), gpooled=new(B, C, dtype=F32))
            rc = L.adil_bn_pool_head_bwd(_ptr(k["g"]), _ptr(k["w"]), _ptr(k["x"]), _ptr(k["pscale"]), _ptr(k["pshift"]),
                                         _ptr(out["gpooled"]), _ptr(out["gx"]), B, HW, C, N, st)
        else:
            raise KeyError(name)
        assert rc == 0, (name, rc)
        if self.keep_log:
            self.log.append((name, kw, out))
        return out


def step_ratios(log):
    """Every logged step of an `Abi` tape against its fp64 restatement on the step's actual inputs (on the CPU): the worst
    max |err| / bound per step name, the bounds being the derived element-wise ones of the reference modules
    (classifier_reference.gaussian_ratio for the stem convolution and the 3x3 steps, dense1x1_reference.gaussian_ratio for
    the 1x1 and transition steps, with dense_block_reference.accumulate where a step accumulates).  The stem's pooling
    pair and the head's gx are bit-defined and compared bit for bit (stem_pool_reference.same_selection / compare_gy,
    dense_head_reference.gaussian_ratios), the pair counting as ratio 0 where it holds."""
    ar, worst, count = R.Arith(), {}, {}
    cpu = lambda v: v.detach().cpu() if isinstance(v, torch.Tensor) else v
    note = lambda name, q: (worst.__setitem__(name, max(worst.get(name, 0.0), q if q == q else float("inf"))),
                            count.__setitem__(name, count.get(name, 0) + 1))
    head = {}
    for name, kw, out in log:
        kw, out = {key: cpu(v) for key, v in kw.items()}, {key: cpu(v) for key, v in out.items()}
        if name.startswith("head"):
            head[name] = (kw, out)
            continue
        ref = restate(ar, name, **kw)
        if name == "pool_fwd":
            B, OH, OW, C = kw["y"].shape
            SP.same_selection("tape pool_fwd", out["p"], out["idx"], ref["p"].float(), ref["idx"], OH, OW)
            note(name, 0.0)
        elif name == "pool_bwd":
            gy, got = ref["_gy"], out["gy"].float()
            on = gy.exact_sum                                          # these have ONE correct value (zeros as values)
            same = R.bits(got + 0.0) == R.bits(gy.want + 0.0)
            assert bool((same | ~on).all()), f"tape pool_bwd: {int((~same & on).sum())} gy elements with an exact sum differ in bits"
            off = ((got.double() - gy.sum * gy.scale.double()).abs() / gy.bound.clamp_min(2.0 ** -126))[~on]
            note(name, float(off.max()) if off.numel() else 0.0)
        elif name in ("stem_fwd", "stem_bwd", "d3_fwd", "d3_bwd"):
            key = "y" if name.endswith("fwd") else "gx"
            note(name, R.gaussian_ratio(out[key], ref["_" + key]))
        else:
            key = "y" if name.endswith("fwd") else "gx"
            note(name, D1.gaussian_ratio(out[key], ref["_" + key]))
    if head:
        (kf, of), (kb, ob) = head["head_fwd"], head["head_bwd"]
        op = DH.Operands(kf["x"], kf["pscale"], kf["pshift"], kf["w"], kf["bias"], kb["g"], None)
        rp, rl, rg = DH.gaussian_ratios("tape head", op, DH.Results(of["pooled"], of["logits"], ob["gpooled"], ob["gx"]))
        note("head_fwd", max(rp, rl))
        note("head_bwd", rg)
    return worst, count


# ---------------------------------------------------------------------------------------------------------------- tape
class Tape(NamedTuple):
    points: list                     # the eight points of `point_names`, NHWC: stem output, block and transition outputs
    pooled: torch.Tensor             # [B][C]
    logits: torch.Tensor             # [B][classes], fp32 on the rounded backends
    grads: Optional[list]            # the gradient entering each of the points, same order and shapes
    grad: Optional[torch.Tensor]     # gradient with respect to the image, NCHW, in the image's dtype on the rounded backends
    mids: list                       # per block, per layer: the bottleneck activation [M][mid] (the ReLU mask of its layer)


def _block_forward(be, layers, x, hit, b):
    """x [B][H][W][C0] -> (the list of features as rows, the mids, what each layer's backward needs)."""
    B, H, W, _ = x.shape
    feats, mids, saved = [_rows(x).contiguous()], [], []
    for i, t in enumerate(layers):
        read = len(feats)
        ps, pb, w, wt = t["pscale"], t["pshift"], t["w"], t.get("wt")
        if hit("short_prefix", b, i):                                  # mutant: a prefix one growth slice too short; the layer's
            assert read >= 2                                           # tables are cut to that width, which keeps the call legal
            read -= 1
            K = sum(f.shape[1] for f in feats[:read])
            ps, pb, w, wt = ps[:K].contiguous(), pb[:K].contiguous(), w[:, :K].contiguous(), None
        xin = torch.cat(feats[:read], 1).contiguous()
        mid = be.step("d1_fwd", x=xin, pscale=ps, pshift=pb, w=w, scale=t["scale"], shift=t["shift"], act=1)["y"]
        out = be.step("d3_fwd", x=mid.reshape(B, H, W, -1), w=t["w3"], wp_fwd=t.get("wp_fwd"))["y"]
        feats.append(_rows(out).contiguous())
        mids.append(mid)
        saved.append(dict(read=read, xin=xin, pscale=ps, pshift=pb, w=w, wt=wt))
    for i in range(len(layers) - 1):
        if hit("swap_slots", b, i):                                    # mutant: two neighbouring layers' output slots exchanged
            feats[i + 1], feats[i + 2] = feats[i + 2], feats[i + 1]
    return feats, mids, saved


def _block_backward(be, layers, saved, mids, g_out, shape, widths, hit, b):
    """g_out [M][Ctot] -> the gradient list (entry 0: the gradient entering the block input, [M][C0])."""
    B, H, W = shape
    G = [t.contiguous() for t in torch.split(g_out, widths, 1)]
    order = range(len(layers) - 1, -1, -1)                             # LAST LAYER FIRST: the specification
    if hit("first_layer_first", b, -1):                                # mutant: the block's backward walks first layer first
        order = range(len(layers))
    for i in order:
        t, s = layers[i], saved[i]
        gmid = be.step("d3_bwd", g=G[i + 1].reshape(B, H, W, -1), w=t["w3"], wp_bwd=t.get("wp_bwd"))["gx"]
        y = mids[i]
        if hit("mask_prev_mid", b, i):                                 # mutant: the mask from the previous layer's mid
            y = mids[i - 1]
        acc = 1
        if hit("no_accumulate", b, i):                                 # mutant: this layer overwrites what the later ones added
            acc = 0
        read = s["read"]
        old = torch.cat(G[:read], 1).contiguous()                      # the gradient of the features the layer read, [M][off_i]
        new = be.step("d1_bwd", g=_rows(gmid), y=y, scale=t["scale"], wt=be.wt(s["w"], s["wt"]), xin=s["xin"], pscale=s["pscale"],
                      pshift=s["pshift"], act=1, accumulate=acc, old=old)["gx"]
        G[:read] = [c.contiguous() for c in torch.split(new, widths[:read], 1)]
    return G


def run_tape(be, tables, x, g_logits, mut=None):
    """x: the image [B][3][H][W], fp32 or bf16 (contiguous NCHW); g_logits: fp32 [B][classes] or None (forward only)."""
    mname, mblock, mlayer = mut if mut is not None else (None, -1, -1)
    hit = lambda name, b, i: mname == name and mblock == b and mlayer == i
    T, step = tables, be.step
    B, _, H, W = x.shape
    s = T["stem"]
    y1 = step("stem_fwd", x=x, w=s["w"], w_fwd=s.get("w_fwd"), mean=T["mean"], inv_std=T["inv_std"], scale=s["scale"],
              shift=s["shift"])["y"]
    o = step("pool_fwd", y=y1)
    p, idx = o["p"], o["idx"]
    points, all_mids, kept = [p], [], []
    h = p
    nb = len(T["blocks"])
    # ---------------------------------------------------------------------------------------------------------- forward
    for b, layers in enumerate(T["blocks"]):
        bb, hh, ww, _ = h.shape
        feats, mids, saved = _block_forward(be, layers, h, hit, b)
        widths = [f.shape[1] for f in feats]
        out = torch.cat(feats, 1).contiguous().reshape(bb, hh, ww, -1)
        points.append(out)
        all_mids.append(mids)
        kept.append(dict(saved=saved, mids=mids, shape=(bb, hh, ww), widths=widths, out=out))
        h = out
        if b != nb - 1:
            t = T["trans"][b]
            xin = out
            if hit("tr_hw_swapped", b, -1):                            # mutant: the transition pools with H and W exchanged
                xin = out.reshape(bb, ww, hh, -1)                      # (the same memory read as a W x H image)
            y = step("tr_fwd", x=xin, pscale=t["pscale"], pshift=t["pshift"], w=t["w"])["y"]
            h = y.reshape(bb, hh // 2, ww // 2, -1)
            kept[-1]["tr_in"] = xin
            points.append(h)
    hd = T["head"]
    bb, hh, ww, C = h.shape
    xh = h.reshape(bb, hh * ww, C)
    if mname == "norm5_twice":                                         # mutant: norm5 in the trunk AND in the head
        xh = be.affine(xh, hd["pscale"], hd["pshift"])
    o = step("head_fwd", x=xh, pscale=hd["pscale"], pshift=hd["pshift"], w=hd["w"], wt=hd.get("wt"), bias=hd["bias"])
    logits, pooled = o["logits"], o["pooled"]
    if g_logits is None:
        return Tape(points, pooled, logits, None, None, all_mids)
    # --------------------------------------------------------------------------------------------------------- backward
    g = step("head_bwd", g=g_logits, w=hd["w"], x=xh, pscale=hd["pscale"], pshift=hd["pshift"])["gx"].reshape(h.shape)
    grads = [None] * len(points)
    at = len(points) - 1
    for b in range(nb - 1, -1, -1):
        kp, layers = kept[b], T["blocks"][b]
        grads[at] = g                                                  # entering the output of block b
        at -= 1
        G = _block_backward(be, layers, kp["saved"], kp["mids"], _rows(g).contiguous(), kp["shape"], kp["widths"], hit, b)
        bb, hh, ww = kp["shape"]
        g_in = G[0]
        if b > 0 and hit("tr_grad_offset", b - 1, -1):                 # mutant: the transition in front reads the gradient buffer
            c0, growth = kp["widths"][0], kp["widths"][1]              # at channel offset `growth` instead of 0
            g_in = torch.cat(G, 1)[:, growth:growth + c0].contiguous()
        g = g_in.reshape(bb, hh, ww, -1)
        grads[at] = g                                                  # entering the block's input: a transition's or the stem's output
        at -= 1
        if b > 0:
            t, kt = T["trans"][b - 1], kept[b - 1]
            xin = kt["tr_in"]
            pb, ph, pw = kt["shape"]
            g = step("tr_bwd", g=g.reshape(xin.shape[0], xin.shape[1] // 2, xin.shape[2] // 2, -1).contiguous(),
                     wt=be.wt(t["w"], t.get("wt")), xin=xin, pscale=t["pscale"], pshift=t["pshift"])["gx"].reshape(pb, ph, pw, -1)
    assert at == -1
    OH, OW = y1.shape[1], y1.shape[2]
    gy = step("pool_bwd", g=g.contiguous(), idx=idx, p=p, scale=s["scale"], OH=OH, OW=OW)["gy"]
    gx = step("stem_bwd", gy=gy, w=s["w"], w_bwd=s.get("w_bwd"), inv_std=T["inv_std"], H=H, W=W,
              out_dtype=BF16 if x.dtype == BF16 else F32)["gx"]
    return Tape(points, pooled, logits, grads, gx, all_mids)


# ------------------------------------------------------------------------------------------------------------ premises
def relu_shares(tape, tables):
    """[(name, share of elements > 0)] of every ReLU behind the stem on a rounded tape: every `mid`, every dense layer's,
    transition's and the head's prologue (pre = x * pscale + pshift, dense1x1_reference.prologue).  (The stem's ReLU sits in
    front of a 3 x 3 maximum: nearly all of its pooled outputs are positive, whatever the statistics.)"""
    ar = R.Arith()
    pos = lambda v: float((v > 0).double().mean())
    cpu = lambda v: v.detach().cpu()
    out = []
    nb = len(tables["blocks"])
    for b, layers in enumerate(tables["blocks"]):
        block = _rows(cpu(tape.points[1 + 2 * b]))
        for i, (t, mid) in enumerate(zip(layers, tape.mids[b])):
            K = t["pscale"].shape[0]
            out.append(("denseblock%d layer %d prologue" % (b + 1, i + 1), pos(D1.prologue(ar, block[:, :K], cpu(t["pscale"]), cpu(t["pshift"]))[0])))
            out.append(("denseblock%d layer %d mid" % (b + 1, i + 1), pos(cpu(mid).double())))
        t = tables["trans"][b] if b != nb - 1 else tables["head"]
        name = "transition%d prologue" % (b + 1) if b != nb - 1 else "head prologue"
        out.append((name, pos(D1.prologue(ar, block, cpu(t["pscale"]), cpu(t["pshift"]))[0])))
    return out


def assert_premises(tape, tables, name=""):
    """What a run must exercise, asserted on the reference tape before any kernel result is looked at: every ReLU share
    inside SHARE, every point finite, the image gradient non-zero in every channel."""
    shares = relu_shares(tape, tables)
    n = sum(len(layers) for layers in tables["blocks"])
    assert len(shares) == 2 * n + len(tables["blocks"])
    for what, share in shares:
        assert SHARE[0] < share < SHARE[1], f"{name}: the ReLU of the {what} keeps {share:.4f} of its elements"
    for what, t in zip(point_names(len(tables["blocks"])), tape.points):
        assert bool(torch.isfinite(t.double()).all()), f"{name}: the {what} is not finite"
    if tape.grad is not None:
        for c in range(3):
            assert float(tape.grad[:, c].double().abs().max()) > 0, f"{name}: the image gradient of channel {c} is zero"
    return shares


# ------------------------------------------------------------------------------------------------------------ networks
def make_inputs(shape, seed=3):
    """(x fp32 [B][3][H][W] in [0, 1], g_logits fp32 [B][classes]): structured images of size 96, cropped."""
    from structured import structured_images
    B, _, H, W = shape
    assert H <= 96 and W <= 96
    images, _ = structured_images(B, classes=4, seed=seed, size=96)
    g = torch.randn(B, CLASSES, generator=torch.Generator().manual_seed(seed + 100))
    return images[:, :, :H, :W].contiguous(), g.contiguous()


def _torch_shares(net, images):
    """The share of positive elements behind every ReLU of the plain fp32 network on `images` (hooks on its BatchNorms)."""
    from dl_attack_on_imagenet_amd import zoo
    shares, hooks = [], []
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            hooks.append(m.register_forward_hook(lambda mod, a, out: shares.append(float((out > 0).float().mean()))))
    with torch.no_grad():
        torch.nn.Sequential(zoo.Normalize(MEAN, STD), net)(images)
    for hk in hooks:
        hk.remove()
    return shares


def make_net(block_config=REAL, seed=5):
    """A zoo.DenseNet (fp32, eval, frozen, 10 classes, growth 32, bottleneck 128): seeded weights, the convolution weights
    rounded to bf16, every BatchNorm randomised by the recipe of tests/test_gpu_dense_block.py::randomised_checkpoint
    (statistics around 0 / 1, gamma of both signs).  If a ReLU of that network keeps a share outside SHARE on the images of
    SHAPES, the running statistics are calibrated on those images instead (one training-mode pass with momentum 1 on the
    first shape, then perturbed channel by channel, gamma of both signs, beta 0.3 N(0,1): mobilenet_tape.make_net's
    recipe).  Returns (net, calibrated)."""
    from dl_attack_on_imagenet_amd import zoo

    def build(calibrate):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            net = zoo.DenseNet(block_config=tuple(block_config), num_classes=CLASSES)
        bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        gen = torch.Generator().manual_seed(seed + 1)
        r = lambda n: torch.randn(n, generator=gen)
        u = lambda n: torch.rand(n, generator=gen)
        sign = lambda n: (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.Conv2d):
                    m.weight.copy_(m.weight.bfloat16().float())
            if calibrate:
                for m in bns:
                    m.momentum = 1.0
                    m.train()
                torch.nn.Sequential(zoo.Normalize(MEAN, STD), net)(make_inputs(SHAPES[0])[0])
                net.eval()
            for m in bns:
                n = m.num_features
                if calibrate:
                    m.momentum = 0.1
                    m.running_mean.mul_(1 + 0.2 * r(n)).add_(0.1 * m.running_var.sqrt() * r(n))
                    m.running_var.mul_(0.6 + 0.8 * u(n))
                    m.weight.copy_((0.7 + 0.6 * u(n)) * sign(n))
                    m.bias.copy_(0.3 * r(n))
                else:
                    m.weight.copy_((0.7 + 0.6 * u(n)) * sign(n))
                    m.bias.copy_(0.2 * r(n))
                    m.running_mean.copy_(0.2 * r(n))
                    m.running_var.copy_(0.6 + 0.8 * u(n))
        for q in net.parameters():
            q.requires_grad_(False)
        return net.eval()

    net = build(False)
    alive = all(SHARE[0] < s < SHARE[1] for shape in SHAPES for s in _torch_shares(net, make_inputs(shape)[0]))
    if alive:
        return net, False
    return build(True), True
