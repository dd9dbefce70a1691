"""The residual stages of a zoo.ResNet as ONE straight-line sequence of C-ABI calls: forward from the pooled stem output p
to the last block's output, and the input gradient back to p, with no autograd.  Written from the contracts of
include/adil_hip.h; every step is one of

    pw_fwd  pw_bwd  join_fwd  join_bwd  conv3x3  conv3x3_bwd  s2_fwd  s2_bwd  affine_act_fwd  affine_act_bwd

with the arguments of the C ABI under the names tests/classifier_reference.py gives them.  Two backends run the very same
tape code:

Abi      each step is one call of the loaded library through ctypes on GPU tensors (bf16 activations, fp32 tables);
Restate  each step is the restatement of that name in classifier_reference over an `Arith`, followed by `finish`.  Over
         `Unrounded` the tape is a plain fp64 function, which tests/test_resnet_wiring_cpu.py holds to the torch modules.

Where the product leaves a gradient sum to autograd (the input of a BasicBlock, and the stage input p feeding conv1 and a
stride-1 downsample) the tape adds in the storage type with `add`: never more than two summands, so no order to get wrong.

Activations are NHWC tensors [B][H][W][C]; pointwise steps see them as rows [B*H*W][C].  `mut` names ONE deliberate wiring
mistake (a (name, block index) pair); the tests assert that each of them is noticed."""
from typing import NamedTuple, Optional

import torch

import classifier_reference as R
from classifier_reference import BF16

JOIN_WIDTHS = (64,)          # the widths at which the product runs a residual join as one kernel
OPS = dict(R.OPS, affine_act_fwd=R.affine_act_fwd, affine_act_bwd=R.affine_act_bwd)       # step name -> restatement


# ------------------------------------------------------------------------------------------------------------- tables
def bn_affine64(bn):
    """Eval-mode BatchNorm as y = x * scale + shift, in fp64 and unrounded."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.double() * scale


def layer_tables(net, affine, device="cpu", wdtype=torch.float64):
    """Per block of layer1..layer4: the convolution weights (1x1 as [N][K], 3x3 as [N][C][3][3]) in `wdtype` and the
    (scale, shift) tables `affine(bn)` gives, on `device`."""
    dev = lambda t: t.detach().to(device)
    wgt = lambda conv: dev(conv.weight).to(wdtype).reshape(conv.weight.shape[:2] if conv.kernel_size == (1, 1)
                                                           else conv.weight.shape).contiguous()
    blocks = []
    for li, layer in enumerate((net.layer1, net.layer2, net.layer3, net.layer4)):
        for bi, blk in enumerate(layer):
            t = dict(stage=li, first=bi == 0, bottleneck=hasattr(blk, "conv3"), down=None)
            convs = ("conv1", "conv2", "conv3") if t["bottleneck"] else ("conv1", "conv2")
            for i, name in enumerate(convs, 1):
                conv, bn = getattr(blk, name), getattr(blk, "bn%d" % i)
                t["w%d" % i] = wgt(conv)
                t["s%d" % i], t["b%d" % i] = (dev(v).contiguous() for v in affine(bn))
            t["stride"] = (blk.conv2 if t["bottleneck"] else blk.conv1).stride[0]
            if blk.downsample is not None:
                sd, bd = (dev(v).contiguous() for v in affine(blk.downsample[1]))
                t["down"] = dict(w=wgt(blk.downsample[0]), s=sd, b=bd, stride=blk.downsample[0].stride[0])
            blocks.append(t)
    return blocks


# ------------------------------------------------------------------------------------------------------------ backends
class Restate:
    """Each step: the restatement of classifier_reference over `ar`, then `finish`."""

    def __init__(self, ar):
        self.ar, self.steps = ar, 0

    def step(self, name, **kw):
        self.steps += 1
        return {k: R.finish(self.ar, o) for k, o in OPS[name](self.ar, **kw).items() if not k.startswith("_")}

    def act(self, t):
        return t.to(self.ar.dtype)

    def add(self, a, b):
        return self.ar.rnd(a + b)


def _transposed(w):
    return w.t()


def _ptr(t):
    import ctypes
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


class Abi:
    """Each step: one call of the loaded library.  `log` keeps (name, arguments, outputs) of every step."""

    def __init__(self, lib, keep_log=False):
        self.lib, self.log, self.keep_log, self._packs = lib, [], keep_log, {}

    def act(self, t):
        return t.to(BF16).contiguous()

    def add(self, a, b):
        return torch.add(a, b)

    def _packed(self, w, how):
        key = (w.data_ptr(), how.__name__)
        if key not in self._packs:
            self._packs[key] = (w, how(w).contiguous())                # keeps w alive: the pointer stays a valid key
        return self._packs[key][1]

    def _wt(self, w):
        return self._packed(w, _transposed)

    def step(self, name, **kw):
        import ctypes
        L = self.lib
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        k = dict(kw)
        for key, v in k.items():
            if isinstance(v, torch.Tensor):
                assert v.is_cuda and v.is_contiguous(), (name, key)
                assert v.dtype == (torch.float32 if "scale" in key or "shift" in key else BF16), (name, key, v.dtype)
        new = lambda *shape: torch.empty(shape, dtype=BF16, device=next(v for v in k.values() if isinstance(v, torch.Tensor)).device)
        if name == "pw_fwd":
            (N, K), M = k["w"].shape, k.get("M") or k["x"].shape[0]
            sub_w, sub_hw = k.get("sub_w", 0), k.get("sub_hw", 0)
            assert k["x"].shape == ((4 * M if sub_w else M), K) and (k.get("res") is None or k["res"].shape == (M, N))
            out = dict(y=new(M, N))
            rc = L.adil_pw_conv_fwd(_ptr(k["x"]), _ptr(k["w"]), _ptr(k["scale"]), _ptr(k["shift"]), _ptr(k.get("res")), _ptr(out["y"]),
                                    M, K, N, int(k.get("relu", 1)), _ptr(k.get("pscale")), _ptr(k.get("pshift")), sub_w, sub_hw, st)
        elif name == "pw_bwd":
            (M, N), K = k["g"].shape, k["wt"].shape[0]
            sub_w, sub_hw = k.get("sub_w", 0), k.get("sub_hw", 0)
            assert k["wt"].shape == (K, N) and (k.get("y") is None or k["y"].shape == (M, N))
            assert k.get("g2") is None or k["g2"].shape == (M, N)
            assert k.get("xin") is None or k["xin"].shape == (M, K)
            if k.get("g3") is not None:
                assert k["g3"].shape == (M // 4, N) and sub_w > 0 and M % (4 * sub_hw) == 0 and sub_hw % sub_w == 0
            out = dict(gx=new(M, K))
            if k.get("want_gres", True):
                out["gres"] = new(M, N)
            rc = L.adil_pw_conv_bwd(_ptr(k["g"]), _ptr(k.get("g2")), _ptr(k.get("y")), _ptr(k["scale"]), _ptr(k["wt"]), _ptr(out["gx"]),
                                    _ptr(out.get("gres")), M, K, N, int(k.get("relu", 1)), _ptr(k.get("xin")), _ptr(k.get("pscale")),
                                    _ptr(k.get("pshift")), _ptr(k.get("g3")), sub_w, sub_hw, st)
        elif name == "join_fwd":
            M, W = k["h2raw"].shape
            C = 4 * W
            assert k["w3"].shape == (C, W) and k["w1"].shape == (W, C) and k["res"].shape == (M, C)
            out = dict(out=new(M, C), h1=new(M, W))
            rc = L.adil_pw_join_fwd(_ptr(k["h2raw"]), _ptr(k["pscale2"]), _ptr(k["pshift2"]), _ptr(k["w3"]), _ptr(k["scale3"]),
                                    _ptr(k["shift3"]), _ptr(k["res"]), _ptr(out["out"]), _ptr(k["w1"]), _ptr(k["scale1"]),
                                    _ptr(k["shift1"]), _ptr(out["h1"]), M, W, C, st)
        elif name == "join_bwd":
            M, W = k["g_h1"].shape
            C = 4 * W
            assert k["wt1"].shape == (C, W) and k["wt3"].shape == (W, C)
            assert k["h1"].shape == (M, W) and k["h2raw"].shape == (M, W) and k["g_out"].shape == (M, C) and k["out"].shape == (M, C)
            out = dict(gres=new(M, C), gx=new(M, W))
            rc = L.adil_pw_join_bwd(_ptr(k["g_h1"]), _ptr(k["h1"]), _ptr(k["scale1"]), _ptr(k["wt1"]), _ptr(k["g_out"]), _ptr(k["out"]),
                                    _ptr(k["scale3"]), _ptr(out["gres"]), _ptr(k["wt3"]), _ptr(k["h2raw"]), _ptr(k["pscale2"]),
                                    _ptr(k["pshift2"]), _ptr(out["gx"]), M, W, C, st)
        elif name in ("conv3x3", "s2_fwd"):
            (B, H, W, C), N = k["x"].shape, k["w"].shape[0]
            assert k["w"].shape == (N, C, 3, 3)
            s2 = name == "s2_fwd"
            assert not s2 or (H % 2 == 0 and W % 2 == 0)
            out = dict(y=new(B, H // 2, W // 2, N) if s2 else new(B, H, W, N))
            fn = L.adil_conv3x3_s2_fwd if s2 else L.adil_conv3x3
            rc = fn(_ptr(k["x"]), _ptr(self._packed(k["w"], R.pack_taps)), _ptr(out["y"]), B, H, W, C, N, st)
        elif name == "conv3x3_bwd":
            (B, H, W, N), C = k["g"].shape, k["w"].shape[1]
            assert k["w"].shape == (N, C, 3, 3)
            out = dict(gx=new(B, H, W, C))
            rc = L.adil_conv3x3(_ptr(k["g"]), _ptr(self._packed(k["w"], R.pack_taps_flipped)), _ptr(out["gx"]), B, H, W, N, C, st)
        elif name == "s2_bwd":
            (B, OH, OW, N), C, H, W = k["g"].shape, k["w"].shape[1], k["H"], k["W"]
            assert k["w"].shape == (N, C, 3, 3) and (H, W) == (2 * OH, 2 * OW)
            out = dict(gx=new(B, H, W, C))
            rc = L.adil_conv3x3_s2_bwd(_ptr(k["g"]), _ptr(self._packed(k["w"], R.pack_taps_bwd_s2)), _ptr(out["gx"]), B, H, W, C, N, st)
        elif name == "affine_act_fwd":
            n = k["x"].numel()
            assert k["dtype"] == BF16 and n % 8 == 0 and (k.get("res") is None or k["res"].numel() == n)
            out = dict(y=new(n))
            rc = L.adil_affine_act_fwd(_ptr(k["x"]), _ptr(k.get("res")), _ptr(k["scale"]), _ptr(k["shift"]), _ptr(out["y"]), n, k["C"],
                                       k["inner"], int(k["relu"]), 1, st)
        elif name == "affine_act_bwd":
            n = k["g"].numel()
            assert k["dtype"] == BF16 and n % 8 == 0 and (k.get("y") is None or k["y"].numel() == n)
            out = dict(gx=new(n))
            if k.get("want_gres", True):
                out["gres"] = new(n)
            rc = L.adil_affine_act_bwd(_ptr(k["g"]), _ptr(k.get("y")), _ptr(k["scale"]), _ptr(out["gx"]), _ptr(out.get("gres")), n,
                                       k["C"], k["inner"], int(k["relu"]), 1, st)
        else:
            raise KeyError(name)
        assert rc == 0, (name, rc)
        if self.keep_log:
            self.log.append((name, kw, out))
        return out


# ---------------------------------------------------------------------------------------------------------------- tape
class Tape(NamedTuple):
    outs: list                       # every block's output, NHWC
    grad: Optional[torch.Tensor]     # gradient with respect to p, NHWC


def _rows(t):
    return t.reshape(-1, t.shape[-1])


def _up2(g, H, W):
    """The zero-filled full-resolution tensor autograd's slice backward makes of a gradient on the stride-2 grid."""
    out = torch.zeros(g.shape[0], H, W, g.shape[3], dtype=g.dtype, device=g.device)
    out[:, ::2, ::2] = g
    return out


def run_tape(be, blocks, p, g=None, joins=True, mut=None):
    """p, g: NHWC.  joins: conv3 of a bottleneck and conv1 of the next run as join_fwd / join_bwd where the product's
    join kernels apply (two bottlenecks of one stage at a width in JOIN_WIDTHS)."""
    mname, mblock = mut if mut is not None else (None, -1)
    hit = lambda name, i: mname == name and mblock == i
    nb = len(blocks)
    joined = [joins and i + 1 < nb and t["bottleneck"] and blocks[i + 1]["bottleneck"] and blocks[i + 1]["down"] is None
              and t["w3"].shape[1] in JOIN_WIDTHS for i, t in enumerate(blocks)]       # block i's conv3 with block i+1's conv1
    x = be.act(p)
    saved, outs, h1 = [], [], None
    # ------------------------------------------------------------------------------------------------------ forward
    for i, t in enumerate(blocks):
        B, H, W, _ = x.shape
        s, d = t["stride"], t["down"]
        OH, OW = H // s, W // s
        if d is None:
            idt = x
        elif d["stride"] == 2:
            src = x.roll(-1, 1) if hit("gather_odd_row", i) else x     # mutant: pixel (2oh+1, 2ow)
            idt = be.step("pw_fwd", x=_rows(src), w=d["w"], scale=d["s"], shift=d["b"], res=None, relu=0, sub_w=OW, sub_hw=OH * OW,
                          M=B * OH * OW)["y"].reshape(B, OH, OW, -1)
        else:
            idt = be.step("pw_fwd", x=_rows(x), w=d["w"], scale=d["s"], shift=d["b"], res=None, relu=0)["y"].reshape(B, H, W, -1)
        conv = "s2_fwd" if s == 2 else "conv3x3"
        if t["bottleneck"]:
            if h1 is None:
                h1 = be.step("pw_fwd", x=_rows(x), w=t["w1"], scale=t["s1"], shift=t["b1"], res=None, relu=1)["y"].reshape(B, H, W, -1)
            raw = be.step(conv, x=h1, w=t["w2"])["y"]
            res = idt
            ps, pb = (t["s1"], t["b1"]) if hit("pre_bn1", i) else (t["s2"], t["b2"])   # mutant: bn1's tables as the prologue
            if joined[i]:
                n = blocks[i + 1]
                o = be.step("join_fwd", h2raw=_rows(raw), pscale2=ps, pshift2=pb, w3=t["w3"], scale3=t["s3"], shift3=t["b3"],
                            res=_rows(res), w1=n["w1"], scale1=n["s1"], shift1=n["b1"])
                out, nxt_h1 = o["out"].reshape(B, OH, OW, -1), o["h1"].reshape(B, OH, OW, -1)
            else:
                out = be.step("pw_fwd", x=_rows(raw), w=t["w3"], scale=t["s3"], shift=t["b3"], res=_rows(res), relu=1, pscale=ps,
                              pshift=pb)["y"].reshape(B, OH, OW, -1)
                nxt_h1 = None
            saved.append(dict(x=x, h1=h1, raw=raw, out=out, ps=ps, pb=pb))
            h1 = nxt_h1
        else:
            C = t["w1"].shape[0]
            raw1 = be.step(conv, x=x, w=t["w1"])["y"]
            h = be.step("affine_act_fwd", x=raw1, scale=t["s1"], shift=t["b1"], res=None, C=C, inner=1, relu=1,
                        dtype=BF16)["y"].reshape(raw1.shape)
            raw2 = be.step("conv3x3", x=h, w=t["w2"])["y"]
            res = h if hit("res_from_main", i) else idt                # mutant: the residual is the main-path tensor
            out = be.step("affine_act_fwd", x=raw2, scale=t["s2"], shift=t["b2"], res=res, C=C, inner=1, relu=1,
                          dtype=BF16)["y"].reshape(raw2.shape)
            saved.append(dict(x=x, h=h, out=out))
        outs.append(out)
        x = out
    if g is None:
        return Tape(outs, None)
    # ----------------------------------------------------------------------------------------------------- backward
    # what arrives at block i's output: g_main (through the next block's main path, or the given gradient), g_skip (the
    # next block's residual gradient, when it has no downsample), g_sub (the gradient of the next block's stride-2
    # downsample input, on the stride-2 grid); a BasicBlock's input gradients were already added into g_main
    g_main, g_skip, g_sub, g_h1_next = be.act(g), None, None, None
    for i in range(nb - 1, -1, -1):
        t, sv = blocks[i], saved[i]
        x, out = sv["x"], sv["out"]
        B, H, W, _ = x.shape
        s, d = t["stride"], t["down"]
        OH, OW = H // s, W // s
        y = saved[i - 1]["out"] if hit("mask_neighbour", i) else out   # mutant: the mask of the block in front
        if t["bottleneck"]:
            if joined[i]:
                n = blocks[i + 1]
                o = be.step("join_bwd", g_h1=_rows(g_h1_next), h1=_rows(saved[i + 1]["h1"]), scale1=n["s1"], wt1=be_wt(be, n["w1"]),
                            g_out=_rows(g_skip), out=_rows(y), scale3=t["s3"], wt3=be_wt(be, t["w3"]), h2raw=_rows(sv["raw"]),
                            pscale2=sv["ps"], pshift2=sv["pb"])
                gres = _rows(g_skip) if hit("join_swap", i) else o["gres"]   # mutant: the join's g_out handed on as its gres
            else:
                g2 = None if hit("drop_g2", i) else g_skip
                g3 = None if hit("drop_g3", i) else g_sub
                kw = {}
                if g3 is not None:                                     # the NEXT block's stride-2 grid, half of this block's output
                    sw = OH // 2 if hit("g3_transposed", i) else OW // 2
                    kw = dict(g3=_rows(g3), sub_w=sw, sub_hw=(OH // 2) * (OW // 2))
                o = be.step("pw_bwd", g=_rows(g_main), wt=be_wt(be, t["w3"]), scale=t["s3"], y=_rows(y),
                            g2=None if g2 is None else _rows(g2), relu=1, xin=_rows(sv["raw"]), pscale=sv["ps"], pshift=sv["pb"],
                            want_gres=True, **kw)
                gres = o["gres"]
            g_raw = o["gx"].reshape(sv["raw"].shape)
            gres = gres.reshape(out.shape)
            if s == 2:
                g_h1 = be.step("s2_bwd", g=g_raw, w=t["w2"], H=H, W=W)["gx"]
            else:
                g_h1 = be.step("conv3x3_bwd", g=g_raw, w=t["w2"])["gx"]
            if i > 0 and joined[i - 1]:
                g_in, g_h1_next = None, g_h1                           # conv1's gradient runs inside the join in front
            else:
                g_in = be.step("pw_bwd", g=_rows(g_h1), wt=be_wt(be, t["w1"]), scale=t["s1"], y=_rows(sv["h1"]), g2=None, relu=1,
                               want_gres=False)["gx"].reshape(x.shape)
                g_h1_next = None
        else:
            C = t["w1"].shape[0]
            o = be.step("affine_act_bwd", g=g_main, y=y, scale=t["s2"], C=C, inner=1, relu=1, dtype=BF16, want_gres=True)
            gres = o["gres"].reshape(out.shape)
            g_h = be.step("conv3x3_bwd", g=o["gx"].reshape(out.shape), w=t["w2"])["gx"]
            g_raw1 = be.step("affine_act_bwd", g=g_h, y=sv["h"], scale=t["s1"], C=C, inner=1, relu=1, dtype=BF16,
                             want_gres=False)["gx"].reshape(g_h.shape)
            if s == 2:
                g_in = be.step("s2_bwd", g=g_raw1, w=t["w1"], H=H, W=W)["gx"]
            else:
                g_in = be.step("conv3x3_bwd", g=g_raw1, w=t["w1"])["gx"]
        # the downsample's input gradient
        g_down = None
        if d is not None:
            g_down = be.step("pw_bwd", g=_rows(gres), wt=be_wt(be, d["w"]), scale=d["s"], y=None, g2=None, relu=0,
                             want_gres=False)["gx"].reshape(B, OH, OW, -1)
        # hand over to the block in front
        if t["bottleneck"] and i > 0:
            g_main, g_skip, g_sub = g_in, (gres if d is None else None), (g_down if d is not None and d["stride"] == 2 else None)
            assert d is None or d["stride"] == 2
        else:                                                          # autograd sums the two gradients of the block input
            other = gres if d is None else (_up2(g_down, H, W) if d["stride"] == 2 else g_down)
            g_main, g_skip, g_sub = be.add(g_in, other), None, None
    return Tape(outs, g_main)


def be_wt(be, w):
    """The transposed copy [K][N] of a pointwise weight [N][K] the gradient calls take."""
    return be._wt(w) if hasattr(be, "_wt") else w.t()


# ------------------------------------------------------------------------------------------------------------ networks
NETWORKS = {"bottleneck": ("Bottleneck", [3, 2, 2, 1]), "basic": ("BasicBlock", [2, 2, 1, 1])}
P_SHAPE = (3, 24, 16, 64)        # NHWC: not square, even down to 6 x 4 in front of the last stride-2 layer; M = 1152, 288, 72, 18


def make_net(kind, seed=11):
    """A small zoo.ResNet (fp32, eval): convolution weights rounded to bf16, BatchNorm statistics randomised with gammas of
    both signs (the recipe of test_fused_stem_module_equals_the_function_bitwise)."""
    from dl_attack_on_imagenet_amd import zoo
    block, layers = NETWORKS[kind]
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = zoo.ResNet(getattr(zoo, block), layers, num_classes=10).eval()
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(m.weight.bfloat16().float())
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_((0.5 + torch.rand(n, generator=gen)) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1))
                m.bias.copy_(0.2 * torch.randn(n, generator=gen))
                m.running_mean.copy_(0.2 * torch.randn(n, generator=gen))
                m.running_var.copy_(0.6 + 0.8 * torch.rand(n, generator=gen))
    for q in net.parameters():
        q.requires_grad_(False)
    return net


def make_inputs(kind, seed=3):
    """(p, g) NHWC bf16 on the CPU: p as a pooled stem emits it (non-negative, no -0.0), g for the last block's output."""
    block, layers = NETWORKS[kind]
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(P_SHAPE, generator=gen).clamp_min(0).to(BF16) + 0.0
    B, H, W, _ = P_SHAPE
    g = torch.randn(B, H // 8, W // 8, 512 * (4 if block == "Bottleneck" else 1), generator=gen).to(BF16)
    return p, g
