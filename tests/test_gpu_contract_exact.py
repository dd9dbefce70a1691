"""The contractions of csrc/adil_contract.hip through dl_attack_on_imagenet_amd.ops against the restatements of
tests/contract_reference.py, on two legs per family:

exact     operands on a grid (narrow, mid, wide one-hot, fp8) on which every product and every partial sum of the kernel
          is an fp32 number: the kernel's bits must EQUAL the float64 restatement rounded once to the stream type;
gaussian  D ~ U[-1, 1], V ~ 0.02 N(0,1), x ~ U[0, 1] against float64, bound derived in contract_reference.gauss_bound;
          the worst err / bound of each row is printed.

Every row is a call of a check_* function of contract_reference.py with a wrapper around ops as `run`;
tests/test_contract_reference_cpu.py calls the same functions with the numpy emulation, so each row is known to pass
for a correct kernel and to fail for the mutants listed there.  Every output sits in a sentinel buffer (Placed of
test_gpu_routes.py) and x is surrounded by NaN: a read outside the tensor that reaches an output shows.
profiles/contract_exact.md lists the rows, the route each reaches and what an MI355X made of them."""
import numpy as np
import pytest
import torch

import contract_reference as C
from test_gpu_routes import ROUTES, SENTINEL, Placed, _id

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def ops():
    from dl_attack_on_imagenet_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().float().cpu().numpy()


def tdtype(stream):
    return BF16 if stream == "bf16" else F32


def nan_placed(src, offset, pad=64):
    """`src` as a contiguous view `offset` elements into a buffer that is NaN everywhere else (before and behind)."""
    n = src.numel()
    buf = torch.full((pad + offset + n + pad,), float("nan"), dtype=src.dtype, device=DEV)
    assert pad * src.element_size() % 16 == 0
    view = buf[pad + offset:pad + offset + n].view(src.shape)
    view.copy_(src)
    assert (view.data_ptr() % 16 != 0) == (offset > 0)
    return view


def sentinel_out(shape, dtype, offset):
    """An output full of NaN inside a sentinel buffer: an element the kernel leaves out stays NaN."""
    return Placed(torch.full(shape, float("nan"), dtype=dtype, device=DEV), offset)


def is_clean(pl):
    return bool((pl.buf[:pl.lo] == SENTINEL).all()) and bool((pl.buf[pl.hi:] == SENTINEL).all())


# -------------------------------------------------------------------------------------------------- wrappers around ops
def run_synth(c):
    o = ops()
    dt = tdtype(c.stream)
    b = c.v.shape[0]
    d = dev(c.d)
    vp = o.pack_codes(dev(c.v), None, b)
    x = None if c.x is None else nan_placed(dev(c.x).to(dt), c.x_off)
    out = sentinel_out((b, c.d.shape[0]), dt, c.out_off)
    kw = dict(delta_clamp=c.delta, pixel_clamp=c.pixel)
    if c.fp8 is not None:
        kw["fp8_absmax"] = c.fp8
        if c.packed:
            kw["d_fp8"] = o.dict_to_fp8(d)
    res = o.synth(x, d, vp, b, out=out.t, out_dtype=dt, **kw)
    assert res.data_ptr() == out.t.data_ptr()
    return dict(out=host(out.t), clean=is_clean(out))


def run_store(store, index, c):
    o = ops()
    dt = tdtype(c.stream)
    b = c.v.shape[0]
    d, st, idx = dev(c.d), dev(store), dev(index)
    vp = o.pack_codes(dev(c.v), None, b)
    out = sentinel_out((b, c.d.shape[0]), dt, 0)
    o.synth_store(st, idx, d, vp, b, dt, out=out.t, delta_clamp=c.delta, pixel_clamp=c.pixel)
    gathered = None
    if dt == F32:
        xg = o.gather_images(st, idx, dtype=F32)
        gathered = host(o.synth(xg, d, vp, b, delta_clamp=c.delta, pixel_clamp=c.pixel))
    return dict(out=host(out.t), gathered=gathered, clean=is_clean(out))


# ------------------------------------------------------------------------------------------------------------- synthesis
# the unaligned placements of test_gpu_routes.ROUTES: x and out in turn off the 16-byte grid, element-wise tiles only
UNALIGNED = [C.SynthRow("bf16" if r.dtype == BF16 else "f32", r.shape[4], r.shape[1] * r.shape[2] * r.shape[3], r.shape[0],
                        r.offset) for r in ROUTES if r.entry == "synth" and r.offset]
assert [_id(r) for r in ROUTES if r.entry == "synth" and r.offset] == [
    "synth-f32-70x3x12x12-K33-off1", "synth-f32-70x3x12x12-K100-off1", "synth-bf16-70x3x12x12-K33-off2",
    "synth-bf16-70x3x12x12-K100-off2"]


def _synth_params(rows):
    return [pytest.param(r, g, id=f"{C.synth_row_id(r)}-{g}") for r in rows for g in C.SYNTH_GRIDS[r.stream]]


@pytest.mark.parametrize("r,grid", _synth_params(C.SYNTH_ROWS + UNALIGNED))
def test_synth_exact(r, grid):
    """adil_synth, five variants (x + V D^T and the pixel clamp: x in the accumulator; the delta clamp, both clamps and
    x = None: the epilogue form) on one exact grid: bits."""
    C.check_synth_exact(r, grid, run_synth)


@pytest.mark.parametrize("kind", C.FP8_KINDS)
@pytest.mark.parametrize("r", C.FP8_ROWS, ids=C.synth_row_id)
def test_synth_fp8_exact(r, kind):
    """adil_synth_fp8 with power-of-two scales: bits; adil_synth_fp8_packed on dict_to_fp8(d): the same bits."""
    C.check_synth_fp8(r, kind, run_synth)


@pytest.mark.parametrize("r", C.SYNTH_GAUSS_ROWS, ids=C.synth_row_id)
def test_synth_gauss(r):
    print(f"\n{C.synth_row_id(r)} gauss: worst err/bound = {C.check_synth_gauss(r, run_synth):.3f}")


@pytest.mark.parametrize("r", C.SYNTH_GAUSS_ROWS, ids=C.synth_row_id)
def test_synth_fp8_gauss(r):
    """adil_synth_fp8 / adil_synth_fp8_packed at fp8_absmax = 8/255: the scales round in fp32."""
    print(f"\n{C.synth_row_id(r)} gauss fp8 (absmax 8/255): worst err/bound = {C.check_synth_gauss(r, run_synth, fp8=True):.4f}")


@pytest.mark.parametrize("r", C.STORE_ROWS, ids=C.synth_row_id)
def test_synth_store(r):
    """adil_synth_store: a store holding every byte, an index with repeated and out-of-order rows."""
    print(f"\n{C.synth_row_id(r)} store: worst err/bound = {C.check_synth_store(r, run_store):.3f}")


# ---------------------------------------------------------------------------------------------------------------- z-step
def _zstep_state(z, m, s, off):
    return [Placed(dev(a), off[n]) for a, n in ((z, "z"), (m, "m"), (s, "s"))]


def run_zstep(z, m, s, dpt, gv, h, lo, hi, dyn, off):
    o = ops()
    b = z.shape[0]
    zf, mf, sf = _zstep_state(z, m, s, off)
    delta = torch.zeros(1, device=DEV)
    dyn_t = torch.tensor(dyn, dtype=torch.float32, device=DEV) if dyn is not None else None
    o.zstep_(zf.t, mf.t, sf.t, dev(dpt), o.pack_codes(dev(gv), None, b), b, o.AdamWScalars(*h), lo, hi, max_abs_delta=delta,
             dyn=dyn_t)
    return dict(z=host(zf.t), m=host(mf.t), s=host(sf.t), delta=float(delta), clean=all(is_clean(t) for t in (zf, mf, sf)))


def run_zstep_codes(z, m, s, dpt, gv, h, lo, hi, dyn, off):
    o = ops()
    b, (p, k) = z.shape[0], dpt.shape
    zf, mf, sf = _zstep_state(z, m, s, off)
    nbytes = o.zstep_codes_slab_bytes(b, p, k)
    assert nbytes > 0
    slabs = Placed(torch.zeros(nbytes // 4, device=DEV), 0)
    stop = o.StopTest(DEV, 1e-6)
    dyn_t = torch.tensor(dyn, dtype=torch.float32, device=DEV) if dyn is not None else None
    vnext = o.zstep_codes_(zf.t, mf.t, sf.t, dev(dpt), o.pack_codes(dev(gv), None, b), b, o.AdamWScalars(*h), lo, hi,
                           slabs.t.view(torch.uint8), stop=stop, dyn=dyn_t)
    assert isinstance(vnext, o.SlabGrad) and vnext.shape == (b, k)
    codes = o.pack_codes(vnext, None, b)
    pad_zero = not bool(codes[b:].any()) and not bool(codes[:, k:].any())
    return dict(z=host(zf.t), m=host(mf.t), s=host(sf.t), delta=float(stop.last_slot()), codes=host(codes[:b, :k]),
                clean=pad_zero and all(is_clean(t) for t in (zf, mf, sf, slabs)))


@pytest.mark.parametrize("grid", ["narrow", "mid"])
@pytest.mark.parametrize("r", C.Z_ROWS, ids=C.zrow_id)
def test_zstep_exact(r, grid):
    """adil_zstep, three steps: gz is exact on the grid, so z, m, s and max |dz| are the bits of adamw_elem_f32 + clamp."""
    C.check_zstep(r, grid, run_zstep)


@pytest.mark.parametrize("r", C.ZC_ROWS, ids=lambda r: C.zrow_id(r).replace("zstep", "zstep_codes"))
def test_zstep_codes_exact(r):
    """adil_zstep_codes: the z-step's bits (and adil_zstep's), the codes of a saturating step to the bit, and the codes of
    a gaussian step against the float64 product of the kernel's own z."""
    worst = C.check_zstep_codes(r, run_zstep_codes, run_zstep)
    print(f"\n{C.zrow_id(r).replace('zstep', 'zstep_codes')} gaussian codes: worst err/bound = {worst:.3f}")
