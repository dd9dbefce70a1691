"""Every launcher branch of the frozen-classifier kernels (csrc/adil_convs.hip, csrc/adil_conv3x3.hip, csrc/adil_stem.hip, affine_act) through
the C ABI against the float64 restatements of tests/classifier_reference.py, on two legs per row:

exact     integer operands, power-of-two scales: the kernel's bits must EQUAL the RNE bf16 rounding of the fp64 value
          (zero mismatching bits, no margin);
gaussian  N(0,1) operands: elementwise |out - r| <= 2^-8 |r| + n 2^-24 S 2 (derived in classifier_reference.py);
          max(err / bound) is printed per row.

In each run the outputs sit between canary elements that must survive, and a second call must give identical bits.
ROUTES names, per row, the kernel instantiation and the tile map (plain, or the XCD swizzle when MT % 8 == 0) it is meant
to reach; PRODUCT is the list of launch signatures FusedResNet-50 / -18 issue at 224 x 224 (every one gets a row), and
test_recorded_calls_are_covered fails with the missing signature when zoo routing changes."""
import ctypes
import json
import os
import time
from ctypes import c_float, c_void_p

import pytest
import torch

import classifier_reference as R
from classifier_reference import BF16, F32, Route

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1

# rows of a 128-row tile map: one partial tile | several tiles, MT % 8 != 0, ragged | MT = 8, ragged | MT = 16
PART, RAG, SW8, SW16 = 77, 461, 929, 2048


def _pwf(branch, M, K, N, **kw):
    return Route("pw_fwd", branch, dict(M=M, K=K, N=N, **kw))


def _pwb(branch, M, K, N, **kw):
    return Route("pw_bwd", branch, dict(M=M, K=K, N=N, **kw))


def _conv(f, branch, B, H, W, C, N):
    return Route(f, branch, dict(B=B, H=H, W=W, C=C, N=N))


ROUTES = [
    # ---- pointwise forward: BN x PRO x RES, relu, K chunks, stride-2 gather, wide N; M classes spread over the rows
    _pwf("pw_conv_fwd_kernel<64,PRO=0,RES=0>: nk=1 (no prefetch), one partial tile", PART, 64, 64),
    _pwf("pw_conv_fwd_kernel<64,PRO=1,RES=0>: NT=3, plain map MT=4 ragged, relu=0", RAG, 128, 192, pro=True, relu=0),
    _pwf("pw_conv_fwd_kernel<64,PRO=1,RES=1>: K=512 (prologue limit), swizzle MT=8 ragged", SW8, 512, 64, pro=True, res=True),
    _pwf("pw_conv_fwd_kernel<64,PRO=0,RES=1>: NT=3, swizzle MT=16", SW16, 128, 192, res=True),
    _pwf("pw_conv_fwd_kernel<128,PRO=0,RES=0>: nk=1, swizzle MT=8 ragged, relu=0", SW8, 64, 128, relu=0),
    _pwf("pw_conv_fwd_kernel<128,PRO=1,RES=0>: K=512, NT=2, swizzle MT=16", SW16, 512, 256, pro=True),
    _pwf("pw_conv_fwd_kernel<128,PRO=1,RES=0>: plain map MT=4 ragged", RAG, 128, 128, pro=True),
    _pwf("pw_conv_fwd_kernel<128,PRO=1,RES=1>: nk=1, plain map MT=4 ragged", RAG, 64, 256, pro=True, res=True),
    _pwf("pw_conv_fwd_kernel<128,PRO=0,RES=1>: one partial tile", PART, 128, 256, res=True),
    _pwf("pw_conv_fwd_kernel<128,PRO=0,RES=1>: K=1024 (16 chunks), plain map", RAG, 1024, 256, res=True),
    _pwf("pw_conv_fwd_kernel<128,PRO=0,RES=0>: K=2048 (32 chunks), swizzle MT=8 ragged", SW8, 2048, 512),
    _pwf("pw_conv_fwd_kernel<128,PRO=0,RES=1>: N=1024 (NT=8), swizzle MT=8 ragged", SW8, 256, 1024, res=True),
    _pwf("pw_conv_fwd_kernel<128,PRO=1,RES=1>: N=2048 (NT=16), K=512, plain map", RAG, 512, 2048, pro=True, res=True),
    _pwf("pw_conv_fwd_kernel<128,PRO=0,RES=0>: stride-2 gather, K=1024, N=2048, one partial tile (1 x 7 x 11)",
         77, 1024, 2048, relu=0, sub=(7, 11)),
    _pwf("pw_conv_fwd_kernel<128,PRO=1,RES=0>: stride-2 gather with prologue, swizzle MT=8 ragged (19 x 7 x 7)",
         931, 128, 128, pro=True, sub=(7, 7)),
    _pwf("pw_conv_fwd_kernel<128,PRO=0,RES=0>: stride-2 gather, swizzle MT=16 (8 x 16 x 16)", 2048, 64, 128, sub=(16, 16)),
    _pwf("pw_conv_fwd_kernel<64,PRO=0,RES=0>: stride-2 gather, plain map (9 x 7 x 7)", 441, 128, 64, relu=0, sub=(7, 7)),
    _pwf("pw_conv_fwd_kernel<128,PRO=0,RES=0>: zero accumulators x negative scales, -0 shifts, relu=1: producers emit +0",
         RAG, 64, 128, zeros=True),
    _pwf("pw_conv_fwd_kernel<64,PRO=0,RES=0>: zero accumulators x negative scales, -0 shifts, relu=0", PART, 64, 64,
         zeros=True, relu=0),
    # ---- pointwise backward: BO x G3, g2, gres (OT > 1: tiles with ot > 0 must not write it), relu, xin, N
    _pwb("pw_conv_bwd_kernel<64,G3=0>: g2 + gres, nn=1, one partial tile", PART, 64, 64, g2=True, gres=True),
    _pwb("pw_conv_bwd_kernel<64,G3=0>: OT=3, xin epilogue, relu=0, swizzle MT=8 ragged", SW8, 192, 128, xin=True, relu=0),
    _pwb("pw_conv_bwd_kernel<64,G3=1>: OT=3, g2 + gres, swizzle MT=8 ragged (5 x 12 x 16)", 960, 192, 64, g2=True, gres=True,
         g3=(6, 8)),
    _pwb("pw_conv_bwd_kernel<64,G3=1>: one partial tile (1 x 6 x 10), relu=0", 60, 64, 128, g3=(3, 5), relu=0),
    _pwb("pw_conv_bwd_kernel<64,G3=0>: N=2048, relu=0, plain map MT=4 ragged", RAG, 64, 2048, relu=0),
    _pwb("pw_conv_bwd_kernel<64,G3=0>: OT=3, gres, swizzle MT=16", SW16, 192, 64, gres=True),
    _pwb("pw_conv_bwd_kernel<128,G3=0>: g2 + gres, swizzle MT=16", SW16, 128, 256, g2=True, gres=True),
    _pwb("pw_conv_bwd_kernel<128,G3=1>: N=1024, OT=2, gres, plain map (3 x 10 x 14)", 420, 256, 1024, gres=True, g3=(5, 7)),
    _pwb("pw_conv_bwd_kernel<128,G3=0>: N=2048, K=512 (OT=4), gres + xin, plain map", RAG, 512, 2048, gres=True, xin=True),
    _pwb("pw_conv_bwd_kernel<128,G3=0>: xin epilogue at K=1024 > 512 (pscale / pshift read from global memory: sound), g2",
         PART, 1024, 256, g2=True, xin=True),
    _pwb("pw_conv_bwd_kernel<128,G3=1>: gres + xin, swizzle MT=16 (2 x 32 x 32)", 2048, 128, 64, gres=True, xin=True, g3=(16, 16)),
    _pwb("pw_conv_bwd_kernel<128,G3=0>: swizzle MT=8 ragged, OT=2, gres, xin", SW8, 256, 64, gres=True, xin=True),
    # ---- residual join, both widths, every M class (one workgroup per 128 rows, no tile map)
    *[Route(f, f"pw_join_kernel<{w},{'BWD' if f == 'join_bwd' else 'FWD'}>: M={m}", dict(M=m, W=w))
      for f in ("join_fwd", "join_bwd") for w in (64, 128) for m in (PART, RAG, SW8, SW16)],
    # ---- conv3x3: <64,4> tiles 256 pixels, <128,2> tiles 128
    _conv("conv3x3", "conv3x3_kernel<64,4>: one partial tile, images (35 px) smaller than the halo", 2, 5, 7, 64, 64),
    _conv("conv3x3", "conv3x3_kernel<64,4>: H=1, W=63 (width limit), C=192", 3, 1, 63, 192, 64),
    _conv("conv3x3", "conv3x3_kernel<64,4>: NT=3, swizzle MT=8 ragged, 40 images of 7 x 7 inside the tiles", 40, 7, 7, 64, 192),
    _conv("conv3x3", "conv3x3_kernel<64,4>: swizzle MT=16, 80 images of 7 x 7", 80, 7, 7, 64, 64),
    _conv("conv3x3", "conv3x3_kernel<64,4>: W=56, plain map MT=2 ragged", 1, 9, 56, 64, 64),
    _conv("conv3x3", "conv3x3_kernel<128,2>: W=1 (a column), one partial tile", 3, 30, 1, 64, 128),
    _conv("conv3x3", "conv3x3_kernel<128,2>: W=2, C=512, images of 6 px", 2, 3, 2, 512, 128),
    _conv("conv3x3", "conv3x3_kernel<128,2>: NT=2, swizzle MT=8 ragged, 20 images of 7 x 7", 20, 7, 7, 128, 256),
    _conv("conv3x3", "conv3x3_kernel<128,2>: swizzle MT=16, 40 images of 7 x 7", 40, 7, 7, 64, 128),
    _conv("conv3x3", "conv3x3_kernel<128,2>: W=63 (width limit), plain map MT=4 ragged", 2, 4, 63, 64, 128),
    _conv("conv3x3", "conv3x3_kernel<128,2>: W=56, C=192, plain map", 1, 8, 56, 192, 128),
    _conv("conv3x3_bwd", "conv3x3_kernel<128,2> on the flipped packing: C=128 <- N=64, swizzle MT=8 ragged", 20, 7, 7, 128, 64),
    _conv("conv3x3_bwd", "conv3x3_kernel<64,4> on the flipped packing: C=64 <- N=128, swizzle MT=8 ragged", 40, 7, 7, 64, 128),
    _conv("conv3x3_bwd", "conv3x3_kernel<64,4> on the flipped packing: W=63, H=1", 2, 1, 63, 64, 64),
    # ---- conv3x3_s2, forward (BN from N) and input gradient (BN from C); rows = B * H/2 * W/2, tiles of 128
    _conv("s2_fwd", "conv3x3_s2_kernel<64,FWD>: OH=OW=1 (W=2), one partial tile", 3, 2, 2, 64, 64),
    _conv("s2_fwd", "conv3x3_s2_kernel<64,FWD>: W=62 (limit), NT=3, plain map MT=2 ragged", 2, 6, 62, 128, 192),
    _conv("s2_fwd", "conv3x3_s2_kernel<64,FWD>: swizzle MT=8 ragged, 19 images of 7 x 7 rows", 19, 14, 14, 64, 64),
    _conv("s2_fwd", "conv3x3_s2_kernel<64,FWD>: swizzle MT=16, 40 images", 40, 14, 14, 64, 64),
    _conv("s2_fwd", "conv3x3_s2_kernel<128,FWD>: OH=1, W=62, C=256", 5, 2, 62, 256, 128),
    _conv("s2_fwd", "conv3x3_s2_kernel<128,FWD>: NT=2, swizzle MT=8 ragged, 19 images", 19, 14, 14, 64, 256),
    _conv("s2_fwd", "conv3x3_s2_kernel<128,FWD>: swizzle MT=16, 40 images", 40, 14, 14, 64, 128),
    _conv("s2_fwd", "conv3x3_s2_kernel<128,FWD>: OW=1 (W=2), one partial tile", 1, 8, 2, 64, 128),
    _conv("s2_bwd", "conv3x3_s2_kernel<64,BWD>: OH=OW=1 (W=2), one partial tile", 3, 2, 2, 64, 64),
    _conv("s2_bwd", "conv3x3_s2_kernel<64,BWD>: W=62 (limit), NT=3, plain map MT=2 ragged", 2, 6, 62, 192, 128),
    _conv("s2_bwd", "conv3x3_s2_kernel<64,BWD>: swizzle MT=8 ragged, 19 images", 19, 14, 14, 64, 64),
    _conv("s2_bwd", "conv3x3_s2_kernel<64,BWD>: swizzle MT=16, 40 images", 40, 14, 14, 64, 128),
    _conv("s2_bwd", "conv3x3_s2_kernel<128,BWD>: OH=1, W=62, N=256", 5, 2, 62, 128, 256),
    _conv("s2_bwd", "conv3x3_s2_kernel<128,BWD>: NT=2, swizzle MT=8 ragged, 19 images", 19, 14, 14, 256, 64),
    _conv("s2_bwd", "conv3x3_s2_kernel<128,BWD>: swizzle MT=16, 40 images", 40, 14, 14, 128, 64),
    _conv("s2_bwd", "conv3x3_s2_kernel<128,BWD>: OW=1 (W=2), one partial tile", 1, 8, 2, 128, 64),
    # ---- the XCD swizzle at the wide channel counts of stages 2 - 4 (B = 512 runs them swizzled): MT = 8, several images
    *[_conv(f, f"{k}: swizzle MT=8 ragged at C={c}, N={n}, {b} images", b, h, h, c, n)
      for f, k, b, h, pairs in (("conv3x3", "conv3x3_kernel<128,2>", 20, 7, ((256, 256), (512, 512))),
                                ("conv3x3_bwd", "conv3x3_kernel<128,2> on the flipped packing", 20, 7, ((256, 256), (512, 512))),
                                ("s2_fwd", "conv3x3_s2_kernel<128,FWD>", 19, 14, ((128, 128), (256, 512), (512, 512))),
                                ("s2_bwd", "conv3x3_s2_kernel<128,BWD>", 19, 14, ((128, 128), (256, 512), (512, 512))))
      for c, n in pairs],
    # ---- stem: both stream dtypes; H/2, W/2 whole 16 x 16 tiles and ragged ones
    *[Route(f, f"{f[:4]}_conv_{f[5:]}_kernel<{'float' if dt == F32 else 'bf16'}>: {what}", dict(B=b, H=h, W=w, dtype=dt))
      for f in ("stem_fwd", "stem_bwd")
      for dt, b, h, w, what in ((F32, 2, 32, 64, "H/2 = 16, W/2 = 32: whole tiles"), (BF16, 2, 32, 64, "H/2 = 16, W/2 = 32: whole tiles"),
                                (F32, 2, 20, 36, "H/2 = 10, W/2 = 18: ragged tiles"), (BF16, 1, 70, 38, "H/2 = 35, W/2 = 19: ragged tiles"))],
    # ---- affine_act: layout 0 (channels_last, C % vec == 0), 1 (inner % vec == 0), 2 (element-wise channel lookup)
    *[Route(f, f"affine_act_{f[4:]}_kernel<{'float,4' if dt == F32 else 'bf16,8'},LAYOUT={lay}>: {what}",
            dict(n=n, C=c, inner=inner, dtype=dt, relu=relu, **{("res" if f == "act_fwd" else "gres"): extra}))
      for f in ("act_fwd", "act_bwd")
      for dt, lay, n, c, inner, relu, extra, what in (
          (BF16, 0, 3200, 64, 1, 1, True, "channels_last"), (BF16, 1, 560, 5, 16, 1, False, "NCHW, inner 16"),
          (BF16, 2, 168, 6, 7, 0, True, "NCHW, inner 7: off the vector width"), (BF16, 2, 120, 12, 1, 1, True, "C = 12: off the vector width"),
          (BF16, 0, 3200, 64, 1, 1, False, "channels_last, no residual"), (BF16, 0, 1280, 128, 1, 0, False, "channels_last, no ReLU"),
          (F32, 0, 3200, 64, 1, 1, True, "channels_last"), (F32, 1, 560, 5, 16, 0, False, "NCHW, inner 16"),
          (F32, 2, 168, 6, 7, 1, True, "NCHW, inner 7: off the vector width"))],
]

# Launch signatures (classifier_reference.call_signature) of FusedResNet-50 and FusedResNet-18, forward + input gradient
# of 64 images of 224 x 224 (the swizzle in stages 1 and 2: pointwise MT = 1568 / 392, conv3x3 784 / 392, stride-2 392), own_strided_conv on / off, chain_joins on / off.  Every one
# gets a kernel-level row below: same K, N, optional pointers, relu, gather, tile and tile map.
PRODUCT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classifier_launch_signatures.json")))


def _product_route(sig):
    entry, f = sig[0], {k: int(v) for k, v in (s.split("=") for s in sig[1:])}
    m = SW8 if f.get("swizzle") else RAG
    branch = "product launch " + " ".join(sig)
    if entry == "adil_pw_conv_fwd":
        sub = (7, 7) if f["gather"] else None
        return _pwf(branch, (931 if f["swizzle"] else 441) if sub else m, f["K"], f["N"], res=bool(f["res"]), pro=bool(f["pro"]),
                    relu=f["relu"], sub=sub)
    if entry == "adil_pw_conv_bwd":
        g3 = ((6, 8) if f["swizzle"] else (5, 7)) if f["g3"] else None
        return _pwb(branch, (960 if f["swizzle"] else 420) if g3 else m, f["K"], f["N"], g2=bool(f["g2"]), gres=bool(f["gres"]),
                    xin=bool(f["xin"]), relu=f["relu"], g3=g3)
    if entry == "adil_conv3x3":              # the call's (C, N); which of the two directions it is does not matter to the kernel
        b = (40 if f["swizzle"] else 11) if f["BN"] == 64 else (20 if f["swizzle"] else 9)
        return _conv("conv3x3", branch, b, 7, 7, f["C"], f["N"])
    if entry in ("adil_conv3x3_s2_fwd", "adil_conv3x3_s2_bwd"):
        return _conv("s2_fwd" if entry.endswith("fwd") else "s2_bwd", branch, 19 if f["swizzle"] else 9, 14, 14, f["C"], f["N"])
    return None                              # join / stem / affine_act signatures are matched by the rows above


ROUTES += [r for r in (_product_route(tuple(s)) for s in PRODUCT) if r is not None]


def row_signature(r):
    """The launch signature of a table row (what call_signature gives for the call the row makes)."""
    return _CALLS[r.family](r, None, None, None, sig=True)


# ----------------------------------------------------------------------------------------------------------- launching
def lib():
    from dl_attack_on_imagenet_amd import _lib
    return _lib.load()


def ptr(t):
    return c_void_p(0 if t is None else t.data_ptr())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


class Canaried:
    """An output tensor between two runs of canary elements."""
    PAD = 512                                # elements: keeps the tensor 16-byte aligned

    def __init__(self, shape, dtype=BF16):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * self.PAD,), R.CANARY, dtype=dtype, device=DEV)
        self.t = self.buf[self.PAD:self.PAD + n].view(shape)

    def intact(self):
        return bool((self.buf[:self.PAD] == R.CANARY).all()) and bool((self.buf[self.PAD + self.t.numel():] == R.CANARY).all())

    def untouched(self):
        return bool((self.buf == R.CANARY).all())


def _code(dt):
    return 0 if dt == F32 else 1


def _call_pw_fwd(r, L, o, outs, sig=False):
    if sig:
        c = r.cfg
        return R.call_signature("adil_pw_conv_fwd", [1, 1, 1, 1, int(bool(c.get("res"))), 1, c["M"], c["K"], c["N"], c.get("relu", 1),
                                                     int(bool(c.get("pro"))), 0, 1 if c.get("sub") else 0, 0])
    M, (N, K) = o["M"], o["w"].shape
    return L.adil_pw_conv_fwd(ptr(o["x"]), ptr(o["w"]), ptr(o["scale"]), ptr(o["shift"]), ptr(o["res"]), ptr(outs["y"].t), M, K, N,
                              o["relu"], ptr(o["pscale"]), ptr(o["pshift"]), o["sub_w"], o["sub_hw"], stream())


def _call_pw_bwd(r, L, o, outs, sig=False):
    if sig:
        c = r.cfg
        return R.call_signature("adil_pw_conv_bwd", [1, int(bool(c.get("g2"))), 1, 1, 1, 1, int(bool(c.get("gres"))), c["M"], c["K"], c["N"],
                                                     c.get("relu", 1), int(bool(c.get("xin"))), 0, 0, int(bool(c.get("g3"))), 0, 0])
    (M, N), K = o["g"].shape, o["wt"].shape[0]
    return L.adil_pw_conv_bwd(ptr(o["g"]), ptr(o["g2"]), ptr(o["y"]), ptr(o["scale"]), ptr(o["wt"]), ptr(outs["gx"].t),
                              ptr(outs["gres"].t if "gres" in outs else None), M, K, N, o["relu"], ptr(o["xin"]), ptr(o["pscale"]),
                              ptr(o["pshift"]), ptr(o["g3"]), o["sub_w"], o["sub_hw"], stream())


def _call_join_fwd(r, L, o, outs, sig=False):
    if sig:
        return R.call_signature("adil_pw_join_fwd", [r.cfg["M"], r.cfg["W"], 4 * r.cfg["W"], 0])
    M, W = o["h2raw"].shape
    return L.adil_pw_join_fwd(ptr(o["h2raw"]), ptr(o["pscale2"]), ptr(o["pshift2"]), ptr(o["w3"]), ptr(o["scale3"]), ptr(o["shift3"]),
                              ptr(o["res"]), ptr(outs["out"].t), ptr(o["w1"]), ptr(o["scale1"]), ptr(o["shift1"]), ptr(outs["h1"].t),
                              M, W, 4 * W, stream())


def _call_join_bwd(r, L, o, outs, sig=False):
    if sig:
        return R.call_signature("adil_pw_join_bwd", [r.cfg["M"], r.cfg["W"], 4 * r.cfg["W"], 0])
    M, W = o["g_h1"].shape
    return L.adil_pw_join_bwd(ptr(o["g_h1"]), ptr(o["h1"]), ptr(o["scale1"]), ptr(o["wt1"]), ptr(o["g_out"]), ptr(o["out"]),
                              ptr(o["scale3"]), ptr(outs["gres"].t), ptr(o["wt3"]), ptr(o["h2raw"]), ptr(o["pscale2"]),
                              ptr(o["pshift2"]), ptr(outs["gx"].t), M, W, 4 * W, stream())


def _call_conv3x3(r, L, o, outs, sig=False):
    c = r.cfg
    if sig:
        return R.call_signature("adil_conv3x3", [0, 0, 0, c["B"], c["H"], c["W"], c["C"], c["N"]])
    return L.adil_conv3x3(ptr(o["x"]), ptr(o["_wp"]), ptr(outs["y"].t), c["B"], c["H"], c["W"], c["C"], c["N"], stream())


def _call_conv3x3_bwd(r, L, o, outs, sig=False):
    c = r.cfg
    if sig:
        return R.call_signature("adil_conv3x3", [0, 0, 0, c["B"], c["H"], c["W"], c["N"], c["C"]])
    return L.adil_conv3x3(ptr(o["g"]), ptr(o["_wp"]), ptr(outs["gx"].t), c["B"], c["H"], c["W"], c["N"], c["C"], stream())


def _call_s2_fwd(r, L, o, outs, sig=False):
    c = r.cfg
    if sig:
        return R.call_signature("adil_conv3x3_s2_fwd", [0, 0, 0, c["B"], c["H"], c["W"], c["C"], c["N"]])
    return L.adil_conv3x3_s2_fwd(ptr(o["x"]), ptr(o["_wp"]), ptr(outs["y"].t), c["B"], c["H"], c["W"], c["C"], c["N"], stream())


def _call_s2_bwd(r, L, o, outs, sig=False):
    c = r.cfg
    if sig:
        return R.call_signature("adil_conv3x3_s2_bwd", [0, 0, 0, c["B"], c["H"], c["W"], c["C"], c["N"]])
    return L.adil_conv3x3_s2_bwd(ptr(o["g"]), ptr(o["_wp"]), ptr(outs["gx"].t), c["B"], c["H"], c["W"], c["C"], c["N"], stream())


def _call_stem_fwd(r, L, o, outs, sig=False):
    c = r.cfg
    if sig:
        return R.call_signature("adil_stem_conv_fwd", [0, _code(c["dtype"])] + [0] * 11 + [c["H"], c["W"]])
    return L.adil_stem_conv_fwd(ptr(o["x"]), _code(c["dtype"]), ptr(o["_wp"]), *(c_float(v) for v in o["mean"]),
                                *(c_float(v) for v in o["inv_std"]), ptr(o["scale"]), ptr(o["shift"]), ptr(outs["y"].t), c["B"],
                                c["H"], c["W"], stream())


def _call_stem_bwd(r, L, o, outs, sig=False):
    c = r.cfg
    if sig:
        return R.call_signature("adil_stem_conv_bwd", [0] * 6 + [_code(c["dtype"]), c["B"], c["H"], c["W"]])
    return L.adil_stem_conv_bwd(ptr(o["gy"]), ptr(o["_wp"]), *(c_float(v) for v in o["inv_std"]), ptr(outs["gx"].t),
                                _code(c["dtype"]), c["B"], c["H"], c["W"], stream())


def _call_act_fwd(r, L, o, outs, sig=False):
    c = r.cfg
    if sig:
        return R.call_signature("adil_affine_act_fwd", [1, int(bool(c.get("res"))), 1, 1, 1, c["n"], c["C"], c["inner"], c["relu"],
                                                        _code(c["dtype"])])
    return L.adil_affine_act_fwd(ptr(o["x"]), ptr(o["res"]), ptr(o["scale"]), ptr(o["shift"]), ptr(outs["y"].t), c["n"], c["C"],
                                 c["inner"], c["relu"], _code(c["dtype"]), stream())


def _call_act_bwd(r, L, o, outs, sig=False):
    c = r.cfg
    if sig:
        return R.call_signature("adil_affine_act_bwd", [1, 1, 1, 1, int(bool(c.get("gres"))), c["n"], c["C"], c["inner"], c["relu"],
                                                        _code(c["dtype"])])
    return L.adil_affine_act_bwd(ptr(o["g"]), ptr(o["y"]), ptr(o["scale"]), ptr(outs["gx"].t),
                                 ptr(outs["gres"].t if "gres" in outs else None), c["n"], c["C"], c["inner"], c["relu"],
                                 _code(c["dtype"]), stream())


_CALLS = {"pw_fwd": _call_pw_fwd, "pw_bwd": _call_pw_bwd, "join_fwd": _call_join_fwd, "join_bwd": _call_join_bwd,
          "conv3x3": _call_conv3x3, "conv3x3_bwd": _call_conv3x3_bwd, "s2_fwd": _call_s2_fwd, "s2_bwd": _call_s2_bwd,
          "stem_fwd": _call_stem_fwd, "stem_bwd": _call_stem_bwd, "act_fwd": _call_act_fwd, "act_bwd": _call_act_bwd}
_PACK = {"conv3x3": R.pack_taps, "conv3x3_bwd": R.pack_taps_flipped, "s2_fwd": R.pack_taps, "s2_bwd": R.pack_taps_bwd_s2,
         "stem_fwd": R.pack_stem_fwd, "stem_bwd": R.pack_stem_bwd}


def to_device(r, o):
    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in o.items()}
    if r.family in _PACK:
        d["_wp"] = _PACK[r.family](d["w"]).contiguous()
    return d


def run_kernel(r, o, ref):
    """One call through the C ABI into canaried outputs shaped like the reference's."""
    outs = {k: Canaried(tuple(v.pre.shape), v.dtype) for k, v in ref.items() if not k.startswith("_")}
    rc = _CALLS[r.family](r, lib(), o, outs)
    torch.cuda.synchronize()
    assert rc == 0, (r.name, rc)
    return outs


LOG = os.environ.get("ADIL_CLASSIFIER_ROUTES_LOG")       # optional: one JSON line per row and leg (profiles/classifier_routes.md)


def _log(**kw):
    if LOG:
        with open(LOG, "a") as f:
            f.write(json.dumps(kw) + "\n")


@pytest.mark.parametrize("r", [pytest.param(r, id=f"{i:03d}-{r.name}"[:90]) for i, r in enumerate(ROUTES)])
def test_classifier_route(r):
    """Both legs of one row: exact leg bit for bit, gaussian leg within the derived bound; canaries intact; a second call
    gives the same bits."""
    t0 = time.time()
    geom = R.geometry(r)
    ref_ar = R.Arith()
    mism, ratio, widened = 0, 0.0, 0.0
    for leg in ("exact", "gaussian"):
        o = to_device(r, R.operands(r, leg))
        ref = R.evaluate(r, ref_ar, {k: v for k, v in o.items() if not k.startswith("_")})
        first = run_kernel(r, o, ref)
        again = run_kernel(r, o, ref)
        for k, c in first.items():
            what = f"{r.name} [{leg}] {k} ({r.branch})"
            assert c.intact(), f"{what}: canary overwritten"
            assert torch.equal(c.buf.view(torch.int16 if c.buf.dtype == BF16 else torch.int32),
                               again[k].buf.view(torch.int16 if c.buf.dtype == BF16 else torch.int32)), f"{what}: second call differs"
            if leg == "exact":
                mism += R.compare_exact(what, c.t, ref[k], geom)
            else:
                q, wf = R.gaussian_ratio(c.t, ref[k]), R.widened_fraction(ref[k])
                ratio, widened = max(ratio, q), max(widened, wf)
                print(f"{what}: max err / bound = {q:.3f}, elements with a rounded-operand allowance: {100 * wf:.2f} %")
                assert q <= 1.0, f"{what}: max err / bound = {q:.3f} > 1"
        if leg == "exact":
            for k, v in ref.items():
                if k.startswith("_"):
                    R.assert_premise(f"{r.name} {k}", v)
    torch.cuda.synchronize()
    _log(row=r.name, branch=r.branch, mismatches=mism, gaussian_ratio=round(ratio, 4), widened=round(widened, 4), seconds=round(time.time() - t0, 3))


# ------------------------------------------------------------------------------------------------------------ refusals
def _refused(fn, *outs):
    rc = fn()
    torch.cuda.synchronize()
    assert rc == EINVAL, rc
    for c in outs:
        assert c.untouched(), "a refused call wrote to its output"


def test_refusals_leave_outputs_untouched():
    """ADIL_EINVAL before any launch: prologue with K > 512, backward N > 2048, conv3x3 W = 64, the stride-2 limits (odd
    H / W, W > 63, C % 64), pscale without pshift (forward) and xin without pscale / pshift (backward)."""
    L = lib()
    z = lambda *s: torch.zeros(s, dtype=BF16, device=DEV)
    f = lambda n: torch.ones(n, device=DEV)
    M = 64
    y = Canaried((M, 64))
    _refused(lambda: L.adil_pw_conv_fwd(ptr(z(M, 576)), ptr(z(64, 576)), ptr(f(64)), ptr(f(64)), None, ptr(y.t), M, 576, 64, 1,
                                        ptr(f(576)), ptr(f(576)), 0, 0, stream()), y)
    _refused(lambda: L.adil_pw_conv_fwd(ptr(z(M, 64)), ptr(z(64, 64)), ptr(f(64)), ptr(f(64)), None, ptr(y.t), M, 64, 64, 1,
                                        ptr(f(64)), None, 0, 0, stream()), y)
    _refused(lambda: L.adil_pw_conv_fwd(ptr(z(M, 64)), ptr(z(64, 64)), ptr(f(64)), ptr(f(64)), None, ptr(y.t), M, 64, 64, 1,
                                        None, ptr(f(64)), 0, 0, stream()), y)
    gx, gres = Canaried((M, 64)), Canaried((M, 2112))
    _refused(lambda: L.adil_pw_conv_bwd(ptr(z(M, 2112)), None, ptr(z(M, 2112)), ptr(f(2112)), ptr(z(64, 2112)), ptr(gx.t), ptr(gres.t),
                                        M, 64, 2112, 1, None, None, None, None, 0, 0, stream()), gx, gres)
    gres = Canaried((M, 64))
    for ps, pb in ((None, f(64)), (f(64), None), (None, None)):
        _refused(lambda: L.adil_pw_conv_bwd(ptr(z(M, 64)), None, ptr(z(M, 64)), ptr(f(64)), ptr(z(64, 64)), ptr(gx.t), ptr(gres.t), M, 64,
                                            64, 1, ptr(z(M, 64)), ptr(ps), ptr(pb), None, 0, 0, stream()), gx, gres)
    y3 = Canaried((1, 2, 64, 64))
    _refused(lambda: L.adil_conv3x3(ptr(z(1, 2, 64, 64)), ptr(z(64, 9, 64)), ptr(y3.t), 1, 2, 64, 64, 64, stream()), y3)
    for (h, w, c, n) in ((4, 64, 64, 64), (3, 4, 64, 64), (4, 6 + 1, 64, 64), (4, 4, 96, 64), (4, 4, 64, 96)):
        ys, gs = Canaried((1, max(h // 2, 1), max(w // 2, 1), n)), Canaried((1, h, w, c))
        _refused(lambda: L.adil_conv3x3_s2_fwd(ptr(z(1, h, w, c)), ptr(z(n, 9, c)), ptr(ys.t), 1, h, w, c, n, stream()), ys)
        _refused(lambda: L.adil_conv3x3_s2_bwd(ptr(z(1, max(h // 2, 1), max(w // 2, 1), n)), ptr(z(c, 9, n)), ptr(gs.t), 1, h, w, c, n,
                                               stream()), gs)
    for w in (64, 128):
        o1, o2 = Canaried((M, 4 * w)), Canaried((M, w))
        _refused(lambda: L.adil_pw_join_fwd(ptr(z(M, w)), ptr(f(w)), ptr(f(w)), ptr(z(4 * w, w)), ptr(f(4 * w)), ptr(f(4 * w)),
                                            ptr(z(M, 4 * w)), ptr(o1.t), ptr(z(w, 4 * w)), ptr(f(w)), ptr(f(w)), ptr(o2.t), M, w, 2 * w,
                                            stream()), o1, o2)


# ---------------------------------------------------------------------------------------------- beyond 2^31 elements
BIG = 2 ** 31


def _need(gb):
    free, _ = torch.cuda.mem_get_info()
    if free < gb * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.0f} GB free, the test needs {gb} GB")


def _ints(shape, amp, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randint(-amp, amp + 1, shape, generator=g, device=DEV, dtype=torch.int8).to(BF16)


def _windows(rows, width):
    """384-row ranges at the start, at the end and around the rows where the element index of a [rows][width] bf16 tensor
    crosses 2^30 (2^31 bytes) and 2^31 (2^32 bytes)."""
    out = [(0, 384)]
    for cross in (2 ** 30, 2 ** 31):
        assert cross // width + 192 < rows
        out.append((cross // width - 192, cross // width + 192))
    return out + [(rows - 384, rows)]


def test_pointwise_beyond_2_31_elements():
    """y, res (forward) and g, gres (backward) of [M][2048] with M 2048 > 2^31, exact leg on row windows."""
    _need(24)
    L, M, K, N = lib(), 2 ** 20 + 300, 64, 2048
    assert M * N > BIG
    G = R.Gen("big-pw", "exact")
    w, scale, shift = G.weight(N, K).to(DEV), G.scale(N).to(DEV), G.shift(N).to(DEV)
    x, res = _ints((M, K), 8, 1), _ints((M, N), 8, 2)
    y = torch.empty(M, N, dtype=BF16, device=DEV)
    assert L.adil_pw_conv_fwd(ptr(x), ptr(w), ptr(scale), ptr(shift), ptr(res), ptr(y), M, K, N, 1, None, None, 0, 0, stream()) == 0
    torch.cuda.synchronize()
    geom = (R.PW_BM, 128, -(-M // R.PW_BM), N // 128)
    for lo, hi in _windows(M, N):
        ref = R.pw_fwd(R.Arith(), x[lo:hi], w, scale, shift, res[lo:hi], 1)
        R.compare_exact(f"pw_fwd rows {lo}..{hi}", y[lo:hi], ref["y"], geom)
    # backward: g = res, mask from y, gres and gx
    wt = G.weight(K, N).to(DEV)
    g = res.clamp(-4, 4)
    gres = torch.empty(M, N, dtype=BF16, device=DEV)
    gx = torch.empty(M, K, dtype=BF16, device=DEV)
    assert L.adil_pw_conv_bwd(ptr(g), None, ptr(y), ptr(scale), ptr(wt), ptr(gx), ptr(gres), M, K, N, 1, None, None, None, None, 0, 0,
                              stream()) == 0
    torch.cuda.synchronize()
    for lo, hi in _windows(M, N):
        ref = R.pw_bwd(R.Arith(), g[lo:hi], wt, scale, y[lo:hi].clamp(-4, 4), relu=1)
        R.compare_exact(f"pw_bwd gres rows {lo}..{hi}", gres[lo:hi], ref["gres"], geom)
        R.compare_exact(f"pw_bwd gx rows {lo}..{hi}", gx[lo:hi], ref["gx"], (R.PW_BM, 64, geom[2], 1))


def test_join_beyond_2_31_elements():
    """out / res / g_out / gres of [M][512] with M 512 > 2^31 (W = 128), exact leg on row windows, forward and backward."""
    _need(24)
    L, M, W = lib(), 2 ** 22 + 300, 128
    C = 4 * W
    assert M * C > BIG
    o = {k: v.to(DEV) for k, v in R.operands(Route("join_fwd", "", dict(M=8, W=W)), "exact").items()}
    o["h2raw"], o["res"] = _ints((M, W), 4, 3), _ints((M, C), 8, 4)
    out, h1 = torch.empty(M, C, dtype=BF16, device=DEV), torch.empty(M, W, dtype=BF16, device=DEV)
    assert L.adil_pw_join_fwd(ptr(o["h2raw"]), ptr(o["pscale2"]), ptr(o["pshift2"]), ptr(o["w3"]), ptr(o["scale3"]), ptr(o["shift3"]),
                              ptr(o["res"]), ptr(out), ptr(o["w1"]), ptr(o["scale1"]), ptr(o["shift1"]), ptr(h1), M, W, C, stream()) == 0
    torch.cuda.synchronize()
    geom = (R.PW_BM, 64, -(-M // R.PW_BM), 1)
    for lo, hi in _windows(M, C):
        ref = R.join_fwd(R.Arith(), **{k: (v[lo:hi] if k in ("h2raw", "res") else v) for k, v in o.items()})
        R.compare_exact(f"join_fwd out rows {lo}..{hi}", out[lo:hi], ref["out"], geom)
        R.compare_exact(f"join_fwd h1 rows {lo}..{hi}", h1[lo:hi], ref["h1"], geom)
    b = {k: v.to(DEV) for k, v in R.operands(Route("join_bwd", "", dict(M=8, W=W)), "exact").items()}
    b["g_h1"], b["g_out"], b["h2raw"] = _ints((M, W), 4, 5), o["res"].clamp(-4, 4), o["h2raw"]
    b["h1"], b["out"] = h1.clamp(0, 3), out.clamp(0, 3)                # ReLU outputs of the forward, as masks
    del o["res"]
    gres, gx = torch.empty(M, C, dtype=BF16, device=DEV), torch.empty(M, W, dtype=BF16, device=DEV)
    assert L.adil_pw_join_bwd(ptr(b["g_h1"]), ptr(b["h1"]), ptr(b["scale1"]), ptr(b["wt1"]), ptr(b["g_out"]), ptr(b["out"]),
                              ptr(b["scale3"]), ptr(gres), ptr(b["wt3"]), ptr(b["h2raw"]), ptr(b["pscale2"]), ptr(b["pshift2"]), ptr(gx),
                              M, W, C, stream()) == 0
    torch.cuda.synchronize()
    rowwise = ("g_h1", "h1", "g_out", "out", "h2raw")
    for lo, hi in _windows(M, C):
        ref = R.join_bwd(R.Arith(), **{k: (v[lo:hi] if k in rowwise else v) for k, v in b.items()})
        R.assert_premise("join_bwd t", ref["_t"])
        R.compare_exact(f"join_bwd gres rows {lo}..{hi}", gres[lo:hi], ref["gres"], geom)
        R.compare_exact(f"join_bwd gx rows {lo}..{hi}", gx[lo:hi], ref["gx"], geom)


@pytest.mark.parametrize("family", ["conv3x3", "s2_fwd", "s2_bwd"])
def test_conv3x3_beyond_2_31_elements(family):
    """The [B][56][56][512] tensor of the call (x; gx for the stride-2 gradient) holds more than 2^31 elements; exact leg
    on whole images at the start, the end and around the 2^30- and 2^31-element crossings."""
    _need(16)
    L, B, H, W, C, N = lib(), 1340, 56, 56, 512, 64
    assert B * H * W * C > BIG and B * H * W < BIG
    w = R.Gen("big-" + family, "exact").weight(N, C, 3, 3).to(DEV)
    if family == "s2_bwd":
        g = _ints((B, H // 2, W // 2, N), 8, 6)
        gx = torch.empty(B, H, W, C, dtype=BF16, device=DEV)
        assert L.adil_conv3x3_s2_bwd(ptr(g), ptr(R.pack_taps_bwd_s2(w)), ptr(gx), B, H, W, C, N, stream()) == 0
    else:
        x = _ints((B, H, W, C), 8, 7)
        oh, ow = (H, W) if family == "conv3x3" else (H // 2, W // 2)
        y = torch.empty(B, oh, ow, N, dtype=BF16, device=DEV)
        fn = L.adil_conv3x3 if family == "conv3x3" else L.adil_conv3x3_s2_fwd
        assert fn(ptr(x), ptr(R.pack_taps(w)), ptr(y), B, H, W, C, N, stream()) == 0
    torch.cuda.synchronize()
    img = H * W * C
    for lo, hi in ((0, 2), (BIG // 2 // img - 1, BIG // 2 // img + 2), (BIG // img - 1, BIG // img + 2), (B - 2, B)):
        if family == "conv3x3":
            R.compare_exact(f"conv3x3 images {lo}..{hi}", y[lo:hi], R.conv3x3(R.Arith(), x[lo:hi], w)["y"])
        elif family == "s2_fwd":
            R.compare_exact(f"s2_fwd images {lo}..{hi}", y[lo:hi], R.conv3x3_s2_fwd(R.Arith(), x[lo:hi], w)["y"])
        else:
            R.compare_exact(f"s2_bwd images {lo}..{hi}", gx[lo:hi], R.conv3x3_s2_bwd(R.Arith(), g[lo:hi], w, H, W)["gx"])


# --------------------------------------------------------------------------------------------- coverage of the product
class Recorder:
    """Stands in for the loaded library: records the launch signature of every classifier-kernel call, then forwards it."""

    def __init__(self, real):
        self.real, self.seen = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith(R.RECORDED_PREFIXES):
            return fn

        def call(*a):
            self.seen.append(R.call_signature(name, a))
            return fn(*a)
        return call


def record_product_signatures(monkeypatch_setattr):
    """Signatures of forward + input gradient of FusedResNet-50 / -18 at 64 x 3 x 224 x 224, all four switch settings."""
    from dl_attack_on_imagenet_amd import _lib, zoo
    rec = Recorder(_lib.load())
    monkeypatch_setattr(_lib, "_lib", rec)
    for name in ("resnet50", "resnet18"):
        for own in (False, True):
            for chain in (True, False):
                net = zoo.build_classifier(name, num_classes=10, seed=1, device=DEV, dtype=BF16, channels_last=True, fuse_bn_act=True,
                                           fuse_stem=True, own_strided_conv=own)
                for m in net.modules():
                    if isinstance(m, zoo.FusedResNet):
                        m.chain_joins = chain
                x = torch.rand(64, 3, 224, 224, generator=torch.Generator().manual_seed(0)).to(DEV).bfloat16().requires_grad_(True)
                torch.autograd.grad(net(x).float().square().sum(), x)
                torch.cuda.synchronize()
                del net
    return sorted(set(rec.seen))


def test_recorded_calls_are_covered(monkeypatch):
    """Every classifier-kernel launch the product makes has a row in ROUTES with the same launch signature."""
    seen = record_product_signatures(monkeypatch.setattr)
    for entry in ("adil_pw_conv_fwd", "adil_pw_conv_bwd", "adil_conv3x3", "adil_conv3x3_s2_fwd", "adil_conv3x3_s2_bwd"):
        assert any(s[0] == entry and "swizzle=1" in s for s in seen), f"{entry} did not reach the swizzle"
    covered = {row_signature(r) for r in ROUTES}
    missing = [s for s in seen if s not in covered]
    assert not missing, "launches of the product without a row in ROUTES:\n" + "\n".join(" ".join(s) for s in missing)
    assert {tuple(s) for s in PRODUCT} == set(seen), "tests/golden/classifier_launch_signatures.json is out of date"
