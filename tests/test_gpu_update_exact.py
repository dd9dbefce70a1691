"""The parameter-update kernels of csrc/adil_update.hip through dl_attack_on_imagenet_amd.ops against the restatements of
tests/update_reference.py, on two legs per family:

exact     operands on an integer grid on which every intermediate of the kernel is exact up to the roundings the model
          names (AdamW: arbitrary gaussian operands, the float32 restatement rounds after every operation exactly as the
          uncontracted kernel does): the kernel's bits must EQUAL the model's, no margin;
gaussian  N(0,1)-derived operands against float64, bound derived in the check's docstring; the worst err / bound of each
          row is printed.

Every row is a call of a check_* function of update_reference.py with a wrapper around ops as `run`;
tests/test_update_reference_cpu.py calls the same functions with numpy emulations of the kernels, so each row is known to
pass for a correct kernel, and to fail for the mutants listed there.  profiles/update_exact.md lists the rows and what
an MI355X made of them."""
import numpy as np
import pytest
import torch

import update_reference as R
from update_reference import F32

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ops():
    from dl_attack_on_imagenet_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


# -------------------------------------------------------------------------------------------------- wrappers around ops
def run_flat(p, g, m, s, h, lo, hi, dyn, fp8):
    o = ops()
    pt, mt, st, gt = dev(p), dev(m), dev(s), g.to(DEV)
    delta = torch.zeros(1, device=DEV)
    dyn_t = torch.tensor(dyn, dtype=torch.float32, device=DEV) if dyn is not None else None
    p8 = torch.full((p.size,), 0xA5, dtype=torch.uint8, device=DEV) if fp8 else None
    o.adamw_clamp_(pt, gt, mt, st, o.AdamWScalars(*h), lo, hi, max_abs_delta=delta, dyn=dyn_t, p_fp8=p8)
    out = dict(p=host(pt), m=host(mt), s=host(st), delta=float(delta))
    if fp8:
        out["fp8"] = host(p8)
    return out


def run_rows(v, m, s, spec, h, radius):
    o = ops()
    vt, mt, st = dev(v), dev(m), dev(s)
    delta = torch.zeros(1, device=DEV)
    pos = dev(spec["pos"]) if spec.get("pos") is not None else None
    if spec["kind"] == "slab":
        buf = dev(spec["slabs"])                                   # caller-owned: the SlabGrad carries no workspace stamp
        g = o.SlabGrad(buf, buf.data_ptr(), spec["nslabs"], spec["rows"], spec["batch"], v.shape[1])
    else:
        g = dev(spec["g"])
    o.adamw_l1ball_(vt, g, pos, mt, st, o.AdamWScalars(*h), radius, max_abs_delta=delta, reset_pos=pos is not None)
    return dict(v=host(vt), m=host(mt), s=host(st), delta=float(delta), pos=None if pos is None else host(pos))


def run_pack(slabs, nslabs, rows, batch, kk):
    o = ops()
    buf = dev(slabs)
    return host(o.pack_codes(o.SlabGrad(buf, buf.data_ptr(), nslabs, rows, batch, kk), None, batch))


def run_l1(x, r, fused):
    o = ops()
    xt = dev(x)
    if not fused:
        o.l1ball_project_(xt, r)
        return host(xt), None
    z, m, s = torch.zeros_like(xt), torch.zeros_like(xt), torch.zeros_like(xt)
    delta = torch.zeros(1, device=DEV)
    o.adamw_l1ball_(xt, z, None, m, s, o.AdamWScalars(*R.IDENTITY_H), r, max_abs_delta=delta)
    assert not bool(m.any()) and not bool(s.any())
    return host(xt), float(delta)


def run_l2(x, r):
    return host(ops().l2ball_project_(dev(x), r))


def run_atom(d, sphere, radius):
    o = ops()
    dt = dev(d)
    norms = o.atom_norms(dt)
    o.atom_l2_project_(dt, sphere=sphere, radius=radius)
    return host(norms), host(dt)


def run_atom_l1(d, r):
    return host(ops().atom_l1_project_(dev(d), r))


def run_ista(v, g, step, lam):
    return host(ops().ista_step_(dev(v), None if g is None else dev(g), step, lam))


def run_spd(a):
    return host(ops().spd_inverse(dev(a)))


def run_metrics(adv, x, misalign):
    at, xt = adv.to(DEV).contiguous(), x.to(DEV).contiguous()
    if misalign:                                                   # one element (4 or 2 bytes) off a 16-byte boundary
        buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)
        view = buf[1:].view(x.shape)
        view.copy_(xt)
        assert view.data_ptr() % 16 == x.element_size() and view.is_contiguous()
        xt = view
    se, sn = ops().image_metrics(at, xt)
    return host(se), host(sn)


# ------------------------------------------------------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", R.ADAMW_N)
def test_adamw_clamp_bits(n, gdtype):
    """adamw_clamp_kernel<GT, false>: p, m, s and max|delta| after each of three steps, clamp to [-0.5, 0.5] and to
    lo == hi; the largest n sends part of the grid round the grid-stride loop a second time."""
    R.check_adamw_flat(n, gdtype, run_flat)


def test_adamw_clamp_device_scalars():
    """The `dyn` route: the host passes bogus step_size / bc2_sqrt, the device buffer holds the right ones."""
    R.check_adamw_flat(1025, torch.float32, run_flat, dyn=True)
    R.check_adamw_flat(7, torch.bfloat16, run_flat, clamps=R.ADAMW_CLAMPS[:1], dyn=True)


@pytest.mark.parametrize("n", R.ADAMW_FP8_N)
def test_adamw_clamp_fp8_copy_bits(n):
    """adamw_clamp_kernel<GT, true>: the same bits, and p_fp8 == e4m3(clamp(256 p_new))."""
    R.check_adamw_flat(n, torch.bfloat16 if n == 1024 else torch.float32, run_flat, clamps=R.ADAMW_CLAMPS[:1], fp8=True)


def test_dict_to_fp8_probe_values():
    """Every finite e4m3 value / 256, every midpoint between neighbours (ties to even) and +-2.0 (saturates)."""
    R.check_fp8(lambda x: host(ops().dict_to_fp8(dev(x))))


@pytest.mark.parametrize("source", R.ROW_SOURCES)
@pytest.mark.parametrize("n,kk", R.ROWS_NK)
def test_adamw_on_code_rows_bits(n, kk, source):
    """adamw_l1ball_ with radius < 0 (AdamW alone), gradient dense / through the slot table / summed from slabs."""
    R.check_adamw_rows(n, kk, source, run_rows)


@pytest.mark.parametrize("nslabs", R.SLAB_COUNTS)
def test_slab_sum_exact(nslabs):
    """slab_sum inside pack_codes and inside adamw_l1ball_: whole rounds of 32, the clamped and weighted tail, a slab of NaN
    behind the last one that must never be read."""
    R.check_slab(nslabs, run_pack, run_rows)


# ------------------------------------------------------------------------------------------------------------ projections
@pytest.mark.parametrize("kk", R.L1_K)
def test_l1ball_exact(kk):
    """l1ball_project_ and the fused adamw_l1ball_ (zero gradient, identity scalars), N in {1, 3, 257}, and radius 0."""
    R.check_l1_exact(kk, run_l1)


@pytest.mark.parametrize("kk", R.L1_GAUSS_K)
def test_l1ball_gauss(kk):
    print(f"\nl1 gauss K={kk}: worst err/bound = {R.check_l1_gauss(kk, run_l1):.3f}")


@pytest.mark.parametrize("kk", R.L2_K)
def test_l2ball_exact_and_gauss(kk):
    R.check_l2_exact(kk, run_l2)
    print(f"\nl2 gauss K={kk}: worst err/bound = {R.check_l2_gauss(kk, run_l2):.3f}")


@pytest.mark.parametrize("p,kk", R.ATOM_SHAPES)
def test_atom_norms_and_scale_exact(p, kk):
    R.check_atom_exact(p, kk, run_atom)


def test_atom_norms_and_scale_gauss():
    print(f"\natom gauss {R.ATOM_GAUSS}: worst err/bound = {R.check_atom_gauss(run_atom):.3f}")


@pytest.mark.parametrize("shape", R.ATOM_L1_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_atom_l1ball_exact(shape):
    R.check_atom_l1_exact(shape, run_atom_l1)


@pytest.mark.parametrize("n", R.ISTA_N)
def test_ista_exact_and_gauss(n):
    R.check_ista_exact(n, run_ista)
    print(f"\nista gauss n={n}: worst err/bound = {R.check_ista_gauss(n, run_ista):.3f}")


# ---------------------------------------------------------------------------------------------- inverse, evaluation sums
@pytest.mark.parametrize("kk", R.SPD_K)
def test_spd_inverse_integer_family(kk):
    R.check_spd(kk, run_spd)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("p", R.METRIC_P)
def test_image_metrics_exact(p, dtype):
    """Vector route (16-byte aligned, P * esz % 16 == 0) and element route (odd sizes, or a misaligned view)."""
    R.check_metrics_exact(p, dtype, run_metrics)
