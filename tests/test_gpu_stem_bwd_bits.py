"""GPU: the stem backward kernels (the quad-form un-pooling and the shift-form 7x7 input gradient) against the recorded bits
of the gather and class forms they replaced (tests/retired_bits.py; the two forms agreed bit for bit when the record was
taken).

recorded bits      adil_stem_pool_bwd and adil_stem_conv_bwd, bit for bit, on the exact and gaussian operands of
                   tests/stem_pool_reference.py and tests/classifier_reference.py (all finite for the convolution; the pooled
                   p of the `synthetic` rows holds NaN and signed zeros, and one more leg gives the un-pooling arbitrary idx
                   bytes), gx in fp32 and bf16, outputs between canaries, prefilled with NaN, every element written.
one-hot g_y1       1.0 at one (oh, ow, co): gx = bf16(w)[co][ci][kh][kw] * inv_std[ci] at (2 oh - 3 + kh, 2 ow - 3 + kw) and
                   zero elsewhere — one fp32 product per element, exact, independent of the record; pins class <-> tap
                   <-> lane."""
from ctypes import c_float, c_void_p

import pytest
import torch

import classifier_reference as R
import retired_bits as RB
import stem_pool_reference as P
from classifier_reference import BF16, F32, Route

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (B, H, W): the smallest image; one whole 16 x 32 tile; one pixel pair past the tile each way; 2 x 2 ragged tiles; odd
# OH = 35 and OW = 19; 3 x 3 whole tiles with an interior one
SHAPES = [(1, 2, 2), (2, 16, 32), (1, 18, 34), (2, 20, 36), (1, 70, 38), (1, 48, 96)]
IDS = ["%dx%dx%d" % s for s in SHAPES]
CONV_LEGS = ("exact", "gaussian")
POOL_LEGS = ("exact", "gaussian", "any idx byte")


def lib():
    from dl_attack_on_imagenet_amd import _lib
    return _lib.load()


def ptr(t):
    return c_void_p(t.data_ptr())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """An output tensor filled with NaN, between two runs of canary elements."""
    PAD = 512

    def __init__(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.buf = torch.full((n + 2 * self.PAD,), P.CANARY, dtype=dtype, device=DEV)
        self.t = self.buf[self.PAD:self.PAD + n].view(shape)
        self.t.fill_(float("nan"))

    def check(self, name):
        assert bool((self.buf[:self.PAD] == P.CANARY).all()) and bool((self.buf[self.PAD + self.n:] == P.CANARY).all()), \
            f"{name}: a canary was overwritten"
        assert not bool(torch.isnan(self.t).any()), f"{name}: {int(torch.isnan(self.t).sum())} elements were not written"


def _conv_bwd(L, gy, wb, inv_std, B, H, W, dt, name):
    gx = Guarded((B, 3, H, W), dt)
    rc = L.adil_stem_conv_bwd(ptr(gy), ptr(wb), *(c_float(s) for s in inv_std), ptr(gx.t), 0 if dt == F32 else 1, B, H, W, stream())
    torch.cuda.synchronize()
    assert rc == 0, (name, rc)
    gx.check(name)
    return gx.t


def _pool_bwd(L, o, B, OH, OW, C, name):
    gy = Guarded((B, OH, OW, C), BF16)
    rc = L.adil_stem_pool_bwd(ptr(o["g"]), ptr(o["idx"]), ptr(o["p"]), ptr(o["scale"]), ptr(gy.t), B, OH, OW, C, stream())
    torch.cuda.synchronize()
    assert rc == 0, (name, rc)
    gy.check(name)
    return gy.t


def conv_case(shape, dt, leg):
    """(case id, inputs in the digest's order, call): call() runs adil_stem_conv_bwd into a fresh guarded gx."""
    B, H, W = shape
    name = f"stem_conv_bwd {B}x{H}x{W} {dt} [{leg}]"
    o = R.operands(Route("stem_bwd", "", dict(B=B, H=H, W=W, dtype=dt)), leg)
    gy, wb = o["gy"].to(DEV).contiguous(), R.pack_stem_bwd(o["w"]).to(DEV).contiguous()
    assert gy.dtype == BF16 and wb.dtype == BF16 and bool(torch.isfinite(gy.float()).all())
    istd = torch.tensor([c_float(s).value for s in o["inv_std"]], dtype=F32)
    return name, [gy, wb, istd], lambda: _conv_bwd(lib(), gy, wb, o["inv_std"], B, H, W, dt, name)


def pool_case(shape, C, leg):
    """As conv_case, for adil_stem_pool_bwd on the pooled grid of an image of `shape`."""
    B, OH, OW = shape[0], shape[1] // 2, shape[2] // 2
    row = P.Row((B, OH, OW, C), "synthetic")
    name = f"stem_pool_bwd {row.name} [{leg}]"
    o = {k: v.to(DEV).contiguous() for k, v in P.operands(row, "gaussian" if leg == "any idx byte" else leg).items()}
    if leg == "any idx byte":
        o["idx"] = torch.randint(0, 256, o["idx"].shape, generator=P.rng(name, "idx"), dtype=torch.int16).to(torch.uint8).to(DEV)
    return name, [o["g"], o["idx"], o["p"], o["scale"]], lambda: _pool_bwd(lib(), o, B, OH, OW, C, name)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_conv_bwd_gives_the_recorded_bits(shape):
    for dt in (F32, BF16):
        for leg in CONV_LEGS:
            name, inputs, call = conv_case(shape, dt, leg)
            assert RB.recorded(name)["nonzero"] > 0, name
            RB.check(name, inputs, call())


@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pool_bwd_gives_the_recorded_bits(shape, C):
    for leg in POOL_LEGS:
        name, inputs, call = pool_case(shape, C, leg)
        if leg != "any idx byte" and (shape[1] // 2) * (shape[2] // 2) > 1:
            assert RB.recorded(name)["nonzero"] > 0, name
        RB.check(name, inputs, call())


# (B, H, W), image, (oh, ow, co): an interior pixel, the four corners' first, the last row and column of an odd grid
ONE_HOT = [((2, 48, 96), 1, (11, 29, 5)), ((2, 48, 96), 0, (8, 16, 63)), ((1, 70, 38), 0, (0, 0, 0)), ((1, 70, 38), 0, (34, 18, 41)),
           ((1, 70, 38), 0, (34, 0, 17)), ((1, 70, 38), 0, (17, 18, 32))]


@pytest.mark.parametrize("shape,img,at", ONE_HOT, ids=["%dx%dx%d-img%d-at%dx%dx%d" % (*s, i, *a) for s, i, a in ONE_HOT])
def test_one_hot_gradient_places_every_tap(shape, img, at):
    L = lib()
    B, H, W = shape
    OH, OW = H // 2, W // 2
    oh, ow, co = at
    w = R.Gen("one-hot stem_bwd", "gaussian").weight(64, 3, 7, 7, fan_in=147)
    wb = R.pack_stem_bwd(w).to(DEV).contiguous()
    inv_std = (1 / 0.229, 1 / 0.224, 1 / 0.225)
    istd32 = torch.tensor([c_float(s).value for s in inv_std], dtype=F32)
    gy = torch.zeros(B, OH, OW, 64, dtype=BF16, device=DEV)
    gy[img, oh, ow, co] = 1.0
    want = torch.zeros(B, 3, H, W, dtype=F32)
    taps = 0
    for kh in range(7):
        for kw in range(7):
            ih, iw = 2 * oh - 3 + kh, 2 * ow - 3 + kw
            if 0 <= ih < H and 0 <= iw < W:
                want[img, :, ih, iw] = w[co, :, kh, kw].float() * istd32
                taps += 1
    assert taps >= 16 and int((want != 0).sum()) == 3 * taps
    for dt in (F32, BF16):
        name = f"one-hot {shape} img {img} at {at} {dt}"
        got = _conv_bwd(L, gy, wb, inv_std, B, H, W, dt, name).cpu()
        ref = want.to(dt)
        bad = got != ref
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}"
