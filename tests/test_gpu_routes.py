"""Every dispatch route of the contractions in csrc/adil_contract.hip against a float64 torch matmul on the device.

adil_synth, adil_grad, adil_zstep and adil_zstep_codes are not single kernels: each launcher picks kernel instantiations
and launch shapes from the stream dtype, the atom tiles grad_at(K) / round_up(K, 16), the batch Bp = round_up(B, 32)
against the row-chunk and "fused while <= 4 chunks" limits, the pixel count (P % 8, % 32, % 64, % 128: FAST tile ranges
and a slow tail) and the 16-byte alignment of the stream pointers.  A wrong slab, row-chunk or atom-half offset in any
of them returns plausible numbers with no error, so ROUTES names, per case, the launcher branch it is meant to reach;
when a dispatch rule changes, this table is where the cases that reach it have to be moved.

Operands are rounded the way the kernels round them (bf16 streams: D and V as bf16; fp32 streams: exact) and the
tolerances are those of the same route family in test_gpu_kernels.py: they scale with sqrt(B) for grad_d and sqrt(P)
for grad_v."""
import zlib
from typing import NamedTuple

import pytest
import torch

from oracle import adil_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SENTINEL = 4096.0            # exact in bf16


class Route(NamedTuple):
    entry: str        # grad (both outputs) | grad_v (want_d=False) | synth | zstep | zstep_codes
    branch: str       # launcher and the condition that selects it
    shape: tuple      # (B, C, H, W, K)
    dtype: torch.dtype
    offset: int = 0   # elements past a 16-byte boundary for the stream pointers the launcher tests (4-byte aligned)
    chunks: int = 1   # grad / grad_v: row chunks of the branch (1 = a deferred grad_v comes back as slabs)


def _round_up(x, m):
    return (x + m - 1) // m * m


def _grad_at(k):
    a = (k + 31) // 32
    return a if a <= 2 else 4


def _zstep_codes_branch(b, k):
    at = (k + 31) // 32                                   # atom_tiles(K); 3 tiles run the 4-tile instantiation
    rb = 2 if at <= 2 and _round_up(b, 32) > 256 else 1
    ny = -(-_round_up(b, 32) // (8 * rb * 32))
    return f"adil_zstep_codes: zstep_codes_kernel<AT={at if at <= 2 else 4}, RB={rb}>, {ny} row range(s) of workgroups"


# --------------------------------------------------------------------------------------------------- the route table
ROUTES = [
    # bf16, 64 < K <= 128, both outputs: the atom-split pass with a slow tail
    Route("grad", "launch_grad_fused_split, slow tail: P%8==0, P%64!=0 (one 512-row chunk, RB=2)", (300, 3, 12, 12, 97), BF16),
    Route("grad", "launch_grad_fused_split, slow tail: P%8==0, P%64!=0; second chunk of 32 rows accumulates (RB=1)",
          (544, 3, 20, 12, 65), BF16, chunks=2),
    Route("grad", "launch_grad_fused_split, slow tail: P%8==0, P%64!=0; three 512-row chunks", (1100, 3, 12, 12, 127), BF16, chunks=3),
    # bf16, K > 64, Bp > 4*512: split off -> grad_d through LDS + generic grad_v, 512-row chunks, a reduce per chunk
    Route("grad", "launch_grad Bp>2048: launch_grad_d_lds + launch_grad_v<bf16,4> generic, fast + slow tail",
          (2080, 3, 12, 12, 100), BF16, chunks=5),
    Route("grad", "launch_grad Bp>2048: launch_grad_d_lds + launch_grad_v<bf16,4> generic, P%64==0, 1-row last chunk",
          (2049, 3, 8, 8, 128), BF16, chunks=5),
    # bf16 grad_v alone at K > 64 (dL/dv = g D of DDrague at 100 atoms)
    Route("grad_v", "launch_grad_v<bf16,4> generic: one 512-row chunk, 16 waves, all FAST", (512, 3, 224, 224, 100), BF16),
    Route("grad_v", "launch_grad_v<bf16,4> generic: chunks of 512 + 96 rows (16 / 4 waves)", (600, 3, 16, 16, 113), BF16, chunks=2),
    # fp32, K > 64, P%32==0: grad_d through grad_fused_f32_kernel (256-row launches), grad_v on the atom-split kernel
    Route("grad", "launch_grad_v_f32<4>: grad_v_f32_kernel<2> k-split, chunks 512 + 96 (r0 offset, reduce per chunk); "
          "launch_grad_fused_f32<4> grad_d only", (600, 3, 16, 16, 100), F32, chunks=2),
    Route("grad", "launch_grad_v_f32<4>: grad_v_f32_kernel<2> k-split, chunks 512 + 512 + 32; "
          "launch_grad_fused_f32<4> grad_d only", (1030, 3, 8, 8, 128), F32, chunks=3),
    # fp32, K > 64, P%32!=0: the generic kernels with FAST ranges and a slow tail
    Route("grad", "launch_grad fp32 AT=4, P%32!=0, P%8==0: launch_grad_d<f32,4> + grad_v_mfma<f32,4,4> "
          "128-row chunks, fast + slow tail", (300, 3, 12, 12, 100), F32, chunks=3),
    # K <= 64 at two atom tiles beyond the fused limit
    Route("grad", "launch_grad bf16 AT=2, Bp>2048 (not fused): launch_grad_d<bf16,2> + grad_v_mfma<bf16,2,16>, "
          "fast + slow tail", (2080, 3, 12, 12, 50), BF16, chunks=5),
    Route("grad", "launch_grad fp32 AT=2, Bp>1024 (not fused): launch_grad_d<f32,2> + launch_grad_v_f32<2> "
          "chunks 512 + 512 + 32", (1030, 3, 16, 16, 50), F32, chunks=3),
    # workgroup shapes picked from the batch: waves per workgroup (NW) and 32-row blocks per wave (RB)
    Route("grad", "launch_grad_fused<bf16,1>: nblk=7 -> NW=8, RB=1; grad_v alone: grad_v_mfma<bf16,1,8>",
          (200, 3, 12, 12, 10), BF16),
    Route("grad", "launch_grad_fused<bf16,1>: nblk=10 -> NW=8, RB=2; grad_v alone: grad_v_mfma<bf16,1,16>",
          (300, 3, 12, 12, 10), BF16),
    Route("grad", "launch_grad_fused<bf16,2>: nblk=7 -> NW=8, RB=1; grad_v alone: grad_v_mfma<bf16,2,8>",
          (200, 3, 12, 12, 50), BF16),
    Route("grad_v", "launch_grad_v<bf16,4> generic: 7 waves -> NW=8", (200, 3, 12, 12, 100), BF16),
    Route("grad", "launch_grad_fused<f32,1> generic (P%32!=0): nblk=7 -> NW=8; grad_v alone: grad_v_mfma<f32,1,8>",
          (200, 3, 12, 12, 10), F32),
    Route("grad", "launch_grad_fused<f32,2> generic (P%32!=0): nblk=7 -> NW=8; grad_v alone: grad_v_mfma<f32,2,8>",
          (200, 3, 12, 12, 50), F32),
    Route("grad_v", "launch_grad_v_f32<1>, P%32==0: grad_v_f32_kernel<1,4> (rows_p <= 128)", (70, 3, 16, 16, 10), F32),
    Route("grad_v", "launch_grad_v_f32<1>, P%32==0: grad_v_f32_kernel<1,8> (128 < rows_p <= 256)", (200, 3, 16, 16, 10), F32),
    Route("grad_v", "launch_grad_v_f32<1>, P%32==0: grad_v_f32_kernel<1,16> (rows_p > 256)", (300, 3, 16, 16, 10), F32),
    Route("grad_v", "launch_grad_v_f32<2>, P%32==0: grad_v_f32_kernel<2,8> (128 < rows_p <= 256)", (200, 3, 16, 16, 50), F32),
    # g not 16-byte aligned: the `vec` test sends every tile through the element-wise kernels
    Route("grad", "launch_grad_fused<bf16,2>, g unaligned: all tiles slow", (70, 3, 12, 12, 50), BF16, offset=2),
    Route("grad", "launch_grad_fused_split, g unaligned: no fast range, slow slabs from 0", (70, 3, 12, 12, 100), BF16, offset=2),
    Route("grad", "launch_grad_fused<f32,2> generic (not grad_fused_f32_kernel), g unaligned: all tiles slow",
          (70, 3, 16, 16, 50), F32, offset=1),
    Route("grad", "launch_grad fp32 AT=4, g unaligned: launch_grad_d<f32,4> + grad_v_mfma<f32,4,4>, all slow",
          (70, 3, 16, 16, 100), F32, offset=1),
    # synth: x / out not 16-byte aligned -> launch_synth_tiles runs no FAST tile
    Route("synth", "launch_synth_tiles, x / out unaligned: element-wise tiles only, Kp<=64", (70, 3, 12, 12, 33), F32, offset=1),
    Route("synth", "launch_synth_tiles, x / out unaligned: element-wise tiles only, Kp>64", (70, 3, 12, 12, 100), F32, offset=1),
    Route("synth", "launch_synth_tiles, x / out unaligned: element-wise tiles only, Kp<=64", (70, 3, 12, 12, 33), BF16, offset=2),
    Route("synth", "launch_synth_tiles, x / out unaligned: element-wise tiles only, Kp>64", (70, 3, 12, 12, 100), BF16, offset=2),
    # adil_zstep (unfused) where DDragueSolver must use it: Kp > 112, with and without a 128-pixel tail
    *[Route("zstep", f"adil_zstep: 8-wave FAST kernel (Kp={_round_up(k, 16)} > 64) + {tail}", (40,) + chw + (k,), F32)
      for k in (113, 120, 128) for chw, tail in (((3, 16, 16), "no tail (P%128==0)"), ((3, 12, 12), "element-wise tail (P%128==48)"))],
    Route("zstep", "adil_zstep, z / m / s unaligned: element-wise tiles only, Kp<=64", (40, 3, 16, 16, 50), F32, offset=1),
    Route("zstep", "adil_zstep, z / m / s unaligned: element-wise tiles only, Kp>64", (40, 3, 16, 16, 120), F32, offset=1),
    # adil_zstep_codes: every atom tiling and both row-block counts
    *[Route("zstep_codes", _zstep_codes_branch(b, k), (b, 3, 16, 16, k), F32)
      for k in (1, 16, 17, 33, 64, 65, 97, 111, 112) for b in (33, 300)],
]

SWEEP_K = (1, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64, 65, 96, 97, 111, 112, 113, 127, 128)


def _sweep_grad_branch(dt, k):
    tail = "fast ranges + slow tail (P%8==0, P%64!=0)"
    if dt == BF16:
        return f"launch_grad_fused_split: {tail}" if k > 64 else f"launch_grad_fused<bf16,{_grad_at(k)}>: {tail}"
    if k > 64:
        return f"launch_grad fp32 AT=4, P%32!=0: launch_grad_d<f32,4> + grad_v_mfma<f32,4,4>: {tail}"
    return f"launch_grad_fused<f32,{_grad_at(k)}> generic (P%32!=0): {tail}"


def _sweep_synth_branch(dt, k):
    kp = _round_up(k, 16)
    variant = (" (HOIST=8)" if dt == BF16 else " (8 waves)") if kp > 64 else ""
    return f"launch_synth_tiles: 3 FAST tiles{variant} + element-wise tail (P%128==48), Kp={kp}"


# the K sweep: one ragged batch, P = 3*12*12 = 432 (a multiple of 8, not of 64 or 128): fast ranges and a tail both run
ROUTES += [Route("grad", _sweep_grad_branch(dt, k), (70, 3, 12, 12, k), dt) for dt in (F32, BF16) for k in SWEEP_K]
ROUTES += [Route("synth", _sweep_synth_branch(dt, k), (70, 3, 12, 12, k), dt) for dt in (F32, BF16) for k in SWEEP_K]


def _id(r):
    b, c, h, w, k = r.shape
    return f"{r.entry}-{'bf16' if r.dtype == BF16 else 'f32'}-{b}x{c}x{h}x{w}-K{k}" + (f"-off{r.offset}" if r.offset else "")


def _routes(*entries):
    return [pytest.param(r, id=_id(r)) for r in ROUTES if r.entry in entries]


# --------------------------------------------------------------------------------------------------- helpers
def ops():
    from dl_attack_on_imagenet_amd import ops as _ops
    return _ops


def close(a, b, tol, what=""):
    """max |a - b| <= tol, computed in float64; the message names the worst element (a slab / chunk offset shows there)."""
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not a.numel():
        return
    diff = (a - b).abs()
    err = float(diff.max())
    if not err <= tol:
        where = tuple(int(i) for i in torch.unravel_index(diff.argmax(), diff.shape))
        raise AssertionError(f"{what}: max error {err:.3e} > {tol:.3e} at {where} (got {float(a[where])}, want {float(b[where])})")


def _gen(r):
    g = torch.Generator(device=DEV)
    g.manual_seed(zlib.crc32(_id(r).encode()))
    return g


class Placed:
    """A contiguous tensor `offset` elements into a buffer whose other elements hold a sentinel: a view at a storage
    offset (not 16-byte aligned for offset > 0) and a check that nothing outside it was written."""

    def __init__(self, src, offset, pad=64):
        n = src.numel()
        self.buf = torch.full((offset + n + pad,), SENTINEL, dtype=src.dtype, device=DEV)
        self.lo, self.hi = offset, offset + n
        self.t = self.buf[offset:offset + n].view(src.shape)
        self.t.copy_(src)
        ptr = self.t.data_ptr()
        assert ptr % 4 == 0 and (ptr % 16 != 0) == (offset > 0), (ptr, offset)

    def untouched(self, what=""):
        assert bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.hi:] == SENTINEL).all()), \
            f"{what}: written outside the tensor"


def _operands(d, v, dt):
    """D and V as the kernels use them, in float64: bf16-rounded for bf16 streams, exact for fp32."""
    if dt == BF16:
        return d.to(BF16).double(), v.to(BF16).double()
    return d.double(), v.double()


def _grad_tol(dt, b, p):
    """(grad_d, grad_v) bounds of the route family: |g| ~ 1, |v| ~ 0.02, |D| <= 1; sums over B resp. P terms."""
    if dt == BF16:
        return 1e-5 * b ** 0.5 * 4, 1e-5 * p ** 0.5 * 4
    return 2e-6 * b ** 0.5 * 4, 3e-6 * p ** 0.5 * 4


# --------------------------------------------------------------------------------------------------- adil_grad
@pytest.mark.parametrize("r", _routes("grad", "grad_v"))
def test_grad_route(r):
    """grad_d = g^T V and grad_v = g D of one route against fp64: both outputs and each alone, accumulation into the
    leading part of a sentinel-filled buffer, codes transposed by pack_codes (vpt=), a deferred grad_v summed by
    pack_codes, and bitwise reproducibility of the route's own call."""
    o = ops()
    b, c, h, w, k = r.shape
    p = c * h * w
    gen = _gen(r)
    d = torch.rand(c, h, w, k, generator=gen, device=DEV) * 2 - 1
    v = torch.randn(b, k, generator=gen, device=DEV) * 0.02
    g = Placed(torch.randn(b, c, h, w, generator=gen, device=DEV).to(r.dtype), r.offset).t
    vp = o.pack_codes(v, None, b)
    vp2, vpt = o.pack_codes(v, None, b, transposed=r.dtype)
    assert torch.equal(vp, vp2)
    dq, vq = _operands(d, v, r.dtype)
    g2 = g.double().reshape(b, p)
    rd = (g2.t() @ vq).reshape(d.shape)
    rv = g2 @ dq.reshape(p, k)
    tol_d, tol_v = _grad_tol(r.dtype, b, p)

    gd, gv = o.grad(g, d, vp, b)
    close(gd, rd, tol_d, "grad_d, both outputs")
    close(gv, rv, tol_v, "grad_v, both outputs")
    gd_only, none = o.grad(g, d, vp, b, want_v=False)
    assert none is None
    close(gd_only, rd, tol_d, "grad_d alone")
    none, gv_only = o.grad(g, d, None, b, want_d=False)
    assert none is None
    close(gv_only, rv, tol_v, "grad_v alone")

    # codes transposed by pack_codes: the same bits as the launch that transposes them itself
    gd_t, gv_t = o.grad(g, d, vp, b, vpt=vpt)
    assert torch.equal(gd_t, gd) and torch.equal(gv_t, gv), "vpt= changed the fused result"
    gd_t, _ = o.grad(g, d, vp, b, want_v=False, vpt=vpt)
    assert torch.equal(gd_t, gd_only), "vpt= changed grad_d alone"

    # accumulation into an existing grad_d that is the leading part of a larger buffer
    init = torch.randn(d.shape, generator=gen, device=DEV) * 0.1
    for want_v in (True, False):
        acc = Placed(init, 0, pad=4096)
        _, gv_acc = o.grad(g, d, vp, b, want_v=want_v, grad_d=acc.t, accumulate_d=True)
        close(acc.t, init.double() + rd, tol_d, f"accumulated grad_d (want_v={want_v})")
        acc.untouched(f"accumulated grad_d (want_v={want_v})")
        if want_v:
            close(gv_acc, rv, tol_v, "grad_v next to an accumulating grad_d")

    # deferred grad_v of the route's own call: slabs when one row chunk covers the batch, summed by pack_codes
    want_d = r.entry == "grad"
    _, lazy = o.grad(g, d, vp if want_d else None, b, want_d=want_d, defer_v=True)
    assert isinstance(lazy, o.SlabGrad) == (r.chunks == 1), (type(lazy), r.chunks)
    got = o.pack_codes(lazy, None, b)[:b, :k] if isinstance(lazy, o.SlabGrad) else lazy
    close(got, rv, tol_v, "deferred grad_v")

    # bitwise reproducibility of the route's own call
    if want_d:
        again = o.grad(g, d, vp, b)
        assert torch.equal(again[0], gd) and torch.equal(again[1], gv)
    else:
        assert torch.equal(o.grad(g, d, None, b, want_d=False)[1], gv_only)


# --------------------------------------------------------------------------------------------------- adil_synth
@pytest.mark.parametrize("r", _routes("synth"))
def test_synth_route(r):
    """out = x + V D^T (x in the accumulator), the +-delta / [0,1] clamped form, and x = None, against fp64; with an
    offset each of x and out in turn sits off the 16-byte grid.  Nothing outside `out` is written; reproducible."""
    o = ops()
    b, c, h, w, k = r.shape
    p = c * h * w
    gen = _gen(r)
    d = torch.rand(c, h, w, k, generator=gen, device=DEV) * 2 - 1
    v = torch.randn(b, k, generator=gen, device=DEV) * 0.02
    x = torch.rand(b, c, h, w, generator=gen, device=DEV).to(r.dtype)
    vp = o.pack_codes(v, None, b)
    dq, vq = _operands(d, v, r.dtype)
    dv = (vq @ dq.reshape(p, k).t()).reshape(x.shape)
    xd = x.double()
    tol = 2 ** -7 if r.dtype == BF16 else 1e-5 * max(1, k ** 0.5)      # bf16: one ulp at magnitude <= 2
    variants = [("x + vD", True, {}, xd + dv),
                ("clamped", True, dict(delta_clamp=0.01, pixel_clamp=True), (xd + dv.clamp(-0.01, 0.01)).clamp(0, 1)),
                ("x=None", False, {}, dv)]
    for what, with_x, kw, ref in variants:
        ref = ref.to(r.dtype).double() if r.dtype == BF16 else ref
        placements = [(0, 0)] if not r.offset else ([(r.offset, 0), (0, r.offset)] if with_x else [(0, r.offset)])
        for x_off, out_off in placements:
            xin = Placed(x, x_off).t if with_x else None
            out = Placed(torch.empty_like(x), out_off)
            first = None
            for _ in range(2):
                res = o.synth(xin, d, vp, b, out=out.t, out_dtype=r.dtype, **kw)
                assert res.data_ptr() == out.t.data_ptr()
                tag = f"{what} (x offset {x_off}, out offset {out_off})"
                close(res, ref, tol, tag)
                out.untouched(tag)
                first = res.clone() if first is None else first
                assert torch.equal(first, res), tag


# --------------------------------------------------------------------------------------------------- adil_zstep
@pytest.mark.parametrize("r", _routes("zstep"))
def test_zstep_route(r):
    """gz = gv D_dagger formed in the kernel + AdamW(z) + clamp + max|dz|, three steps, against the explicit fp64
    sequence (bounds of test_zstep_fused_vs_unfused); with an offset each of z, m, s in turn is off the 16-byte grid."""
    o = ops()
    b, c, h, w, k = r.shape
    p = c * h * w
    gen = _gen(r)
    dpt = torch.randn(c, h, w, k, generator=gen, device=DEV) * 0.1
    gv = torch.randn(b, k, generator=gen, device=DEV)
    z0 = torch.randn(b, c, h, w, generator=gen, device=DEV) * 0.01
    eps = 0.02
    for moved in (("z", "m", "s") if r.offset else (None,)):
        off = {n: (r.offset if n == moved else 0) for n in "zms"}
        zf, mf, sf = Placed(z0, off["z"]), Placed(torch.zeros_like(z0), off["m"]), Placed(torch.zeros_like(z0), off["s"])
        zr = z0.double().clone()
        st = O.AdamWState(zr, 1e-2)
        sched = o.AdamWSchedule(1e-2)
        delta = torch.zeros(1, device=DEV)
        for it in range(3):
            gvi = gv * 0.5 ** it
            gz = (gvi.double() @ dpt.double().reshape(p, k).t()).reshape(z0.shape)
            prev = zr.clone()
            st.step(zr, gz)
            zr.clamp_(-eps, eps)
            delta.zero_()
            o.zstep_(zf.t, mf.t, sf.t, dpt, o.pack_codes(gvi, None, b), b, sched.next(), -eps, eps, max_abs_delta=delta)
            tag = f"it {it}, {moved or 'nothing'} unaligned"
            # the first AdamW steps are ~ lr*g/(|g|+1e-8): elements with |gz| ~ 1e-7 amplify the fp32 rounding of gz
            close(zf.t, zr, 5e-5, f"z {tag}")
            assert float((zf.t.double() - zr).abs().mean()) <= 1e-7, tag
            assert abs(float(delta) - float((zr - prev).abs().max())) <= 5e-5, tag
        close(mf.t, st.m, 1e-5, "m")
        close(sf.t, st.v, 1e-5, "s")
        for t, n in ((zf, "z"), (mf, "m"), (sf, "s")):
            t.untouched(n)


# --------------------------------------------------------------------------------------------------- adil_zstep_codes
@pytest.mark.parametrize("r", _routes("zstep_codes"))
def test_zstep_codes_route(r):
    """The z-step that also leaves the next codes: z, m, s and the stop slots bit for bit those of adil_zstep, and the
    codes pack_codes sums from the slabs equal z_new D_dagger^T of an fp64 matmul."""
    o = ops()
    b, c, h, w, k = r.shape
    p = c * h * w
    gen = _gen(r)
    dpt = torch.randn(c, h, w, k, generator=gen, device=DEV) * 0.1
    gv = torch.randn(b, k, generator=gen, device=DEV)
    z0 = torch.randn(b, c, h, w, generator=gen, device=DEV) * 0.01
    eps = 0.02
    nbytes = o.zstep_codes_slab_bytes(b, p, k)
    assert nbytes > 0
    slabs = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    za, zb = z0.clone(), z0.clone()
    ma, sa, mb, sb = (torch.zeros_like(z0) for _ in range(4))
    sched_a, sched_b = o.AdamWSchedule(1e-2), o.AdamWSchedule(1e-2)
    stop_a, stop_b = o.StopTest(DEV, 1e-6), o.StopTest(DEV, 1e-6)
    for it in range(2):
        gvp = o.pack_codes(gv * 0.5 ** it, None, b)
        o.zstep_(za, ma, sa, dpt, gvp, b, sched_a.next(), -eps, eps, stop=stop_a)
        vnext = o.zstep_codes_(zb, mb, sb, dpt, gvp, b, sched_b.next(), -eps, eps, slabs, stop=stop_b)
        assert torch.equal(za, zb) and torch.equal(ma, mb) and torch.equal(sa, sb), it
        assert torch.equal(stop_a.slots, stop_b.slots), it
        assert isinstance(vnext, o.SlabGrad) and vnext.shape == (b, k)
        codes = o.pack_codes(vnext, None, b)
        ref = zb.double().reshape(b, p) @ dpt.double().reshape(p, k)
        close(codes[:b, :k], ref, 2e-6 * float(ref.abs().max()), f"codes it {it}")
        assert not bool(codes[b:].any()) and not bool(codes[:, k:].any())


def _zstep_codes_rc(z, m, s, dpt, gvp, b, p, k, slabs):
    """adil_zstep_codes called directly (the ops wrapper refuses some shapes before the library sees them)."""
    from ctypes import byref, c_int, c_void_p
    o = ops()
    h = o.AdamWSchedule(1e-2).next()
    n = c_int(-7)
    from dl_attack_on_imagenet_amd import _lib
    rc = _lib.load().adil_zstep_codes(
        c_void_p(z.data_ptr()), c_void_p(m.data_ptr()), c_void_p(s.data_ptr()), c_void_p(dpt.data_ptr()),
        c_void_p(gvp.data_ptr()), b, p, k, h.decay, h.b1, h.b2, h.eps, h.step_size, h.bc2_sqrt, -1.0, 1.0, None, None, 0.0,
        None, None, c_void_p(slabs.data_ptr()), slabs.numel(), byref(n), c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, n.value


@pytest.mark.parametrize("b", [33, 300])
def test_zstep_codes_refuses_k113_and_unaligned_z(b):
    """K = 113 (Kp = 128 > 112) reports 0 slab bytes and is refused by the wrapper AND by the library, which writes
    nothing; a z off the 16-byte grid is refused (ADIL_EINVAL) instead of run."""
    from dl_attack_on_imagenet_amd import _lib
    o = ops()
    c, h, w = 3, 16, 16
    p = c * h * w
    gen = torch.Generator(device=DEV)
    gen.manual_seed(b)
    k = 113
    assert o.zstep_codes_slab_bytes(b, p, k) == 0 and o.zstep_codes_slab_bytes(b, p, 112) > 0
    dpt = torch.randn(c, h, w, k, generator=gen, device=DEV) * 0.1
    z0 = torch.randn(b, c, h, w, generator=gen, device=DEV) * 0.01
    gvp = o.pack_codes(torch.randn(b, k, generator=gen, device=DEV), None, b)
    z, m, s = z0.clone(), torch.zeros_like(z0), torch.zeros_like(z0)
    slabs = torch.full((2 * o.zstep_codes_slab_bytes(b, p, 112),), 7, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        o.zstep_codes_(z, m, s, dpt, gvp, b, o.AdamWSchedule(1e-2).next(), -1.0, 1.0, slabs)
    rc, n = _zstep_codes_rc(z, m, s, dpt, gvp, b, p, k, slabs)
    assert rc == -1 and n == 0, (rc, n)                                   # ADIL_EINVAL, no slabs reported
    assert torch.equal(z, z0) and not bool(m.any()) and not bool(s.any()) and bool((slabs == 7).all())

    k = 64
    dpt = torch.randn(c, h, w, k, generator=gen, device=DEV) * 0.1
    gvp = o.pack_codes(torch.randn(b, k, generator=gen, device=DEV), None, b)
    zu = Placed(z0, 1)
    m, s = torch.zeros_like(z0), torch.zeros_like(z0)
    slabs = torch.full((o.zstep_codes_slab_bytes(b, p, k),), 7, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.AdilLibraryError, match="EINVAL"):
        o.zstep_codes_(zu.t, m, s, dpt, gvp, b, o.AdamWSchedule(1e-2).next(), -1.0, 1.0, slabs)
    torch.cuda.synchronize()
    assert torch.equal(zu.t, z0) and not bool(m.any()) and not bool(s.any()) and bool((slabs == 7).all())
    zu.untouched("z")
