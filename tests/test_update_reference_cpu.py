"""tests/update_reference.py checked without a GPU:

* every restatement against torch / the oracle in float64;
* how far the kernel's AdamW (weights 1.0f - b formed in fp32) sits from torch.optim.AdamW, against a derived bound;
* every row of tests/test_gpu_update_exact.py run through the numpy emulation of its kernel, through the very check
  function the GPU file uses: the rows are known to pass for a correct kernel before anyone has a GPU;
* the exact legs reject every mutant (a deliberately wrong kernel variant);
* vacuity: the row sets contain the cases they are meant to contain, asserted on the reference alone.
"""
import numpy as np
import pytest
import torch

import update_reference as R
from oracle import adil_oracle as O
from update_reference import F32, U


# ------------------------------------------------------------------------------------------------- emulation "wrappers"
def run_flat(mutant=None):
    def run(p, g, m, s, h, lo, hi, dyn, fp8):
        if dyn is not None:                                          # the device scalars win over the host's
            h = h[:4] + tuple(dyn)
        out = R.emu_adamw_flat(p, g, m, s, h, lo, hi, mutant)
        if fp8:
            out["fp8"] = R.fp8_bytes(out["p"], 128.0 if mutant == "fp8_scale_128" else 256.0)
        return out
    return run


def dense_gradient(spec, n, kk, mutant=None):
    if spec["kind"] == "dense":
        return spec["g"]
    if spec["kind"] == "pos":
        gb = spec["g"]
    else:
        gb = R.emu_slab_sum(spec["slabs"], spec["nslabs"], mutant)
    pos = spec["pos"] if spec["pos"] is not None else np.arange(n)
    g = np.zeros((n, kk), F32)
    for row in range(n):
        if pos[row] >= 0:
            g[row] = gb[pos[row]]
    return g


def run_rows(mutant=None):
    def run(v, m, s, spec, h, radius):
        n, kk = v.shape
        out = R.emu_adamw_rows(v, dense_gradient(spec, n, kk, mutant), m, s, h, radius, mutant)
        out["pos"] = np.full(n, -1, np.int32)
        return out
    return run


def run_pack(mutant=None):
    def run(slabs, nslabs, rows, batch, kk):
        vp = np.zeros(((batch + 31) // 32 * 32, (kk + 15) // 16 * 16), F32)
        vp[:batch, :kk] = R.emu_slab_sum(slabs, nslabs, mutant)[:batch]
        return vp
    return run


def run_l1(mutant=None):
    def run(x, r, fused):
        if not fused:
            return R.emu_l1ball(x, r, mutant), None
        z = np.zeros_like(x)
        out = R.emu_adamw_rows(x, z, z, z, R.IDENTITY_H, r, mutant)
        return out["v"], out["delta"]
    return run


def run_atom(mutant=None):
    return lambda d, sphere, radius: R.emu_atom_project(d, sphere, radius, mutant)


def run_metrics(mutant=None):
    return lambda adv, x, misalign: R.emu_image_metrics(adv, x, mutant)


# ------------------------------------------------------------------------------------------ restatements against torch
def test_adamw_restatement_is_torch_adamw_in_float64():
    gen = torch.Generator().manual_seed(0)
    p0 = torch.randn(5000, generator=gen, dtype=torch.float64)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=0.01)
    p, m, s = p0.numpy().copy(), np.zeros(5000), np.zeros(5000)
    for t in range(1, 4):
        g = torch.randn(5000, generator=gen, dtype=torch.float64)
        ref.grad = g.clone()
        opt.step()
        p, m, s = R.adamw_torch64(p, g.numpy(), m, s, 0.01, t)
        assert np.abs(p - ref.detach().numpy()).max() <= 1e-14
    st = opt.state[ref]
    assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-15 and np.abs(s - st["exp_avg_sq"].numpy()).max() <= 1e-15


def test_adamw_hyper_is_the_schedule_of_ops():
    from dl_attack_on_imagenet_amd import ops
    sched = ops.AdamWSchedule(0.01)
    for t in range(1, 5):
        h = sched.next()
        assert (h.decay, h.b1, h.b2, h.eps, h.step_size, h.bc2_sqrt) == R.adamw_hyper(0.01, t)


def test_adamw_kernel_weights_deviate_from_torch_by_a_bounded_amount():
    """The kernel forms its weights as 1.0f - b in fp32: 1.0f - 0.999f = 0.00099998713 where torch uses 0.001 (relative
    d2 = 1.3e-5), 1.0f - 0.9f = 0.100000024 (d1 = 2.4e-7).  s scales with (1 - d2), so sqrt(s) moves by d2 / 2 and the
    update by (d2 / 2 + d1) of itself; ten fp32 roundings sit on the update chain and two on p (decay, subtraction).
    Per step, elementwise, with the float64 torch trajectory as reference:
        bound_t = bound_{t-1} + |update_t| (d2 / 2 + d1 + 10 u) + 2 u |p_t|.
    The measured maximum is what include/adil_hip.h and DESIGN.md quote."""
    d2 = abs(float(F32(1) - F32(0.999)) / 0.001 - 1.0)
    d1 = abs(float(F32(1) - F32(0.9)) / 0.1 - 1.0)
    assert 1.2e-5 < d2 < 1.4e-5 and d1 < 3e-7
    rng = np.random.default_rng(0)
    n = 100000
    p32 = rng.standard_normal(n).astype(F32)
    m32, s32 = np.zeros(n, F32), np.zeros(n, F32)
    p64, m64, s64 = p32.astype(np.float64), np.zeros(n), np.zeros(n)
    bound = np.zeros(n)
    worst_abs = worst_ratio = 0.0
    differ = 0.0
    ref = torch.nn.Parameter(torch.from_numpy(p32.copy()))
    opt = torch.optim.AdamW([ref], lr=0.01)
    for t in range(1, 4):
        g = rng.standard_normal(n).astype(F32)
        p32, m32, s32, _, _ = R.adamw_elem_f32(p32, g, m32, s32, R.adamw_hyper(0.01, t))
        new64, m64, s64 = R.adamw_torch64(p64, g, m64, s64, 0.01, t)
        upd = np.abs(new64 - p64 * (1.0 - 0.01 * 1e-2))
        p64 = new64
        bound = bound + upd * (d2 / 2 + d1 + 10 * U) + 2 * U * np.abs(p64)
        err = np.abs(p32.astype(np.float64) - p64)
        worst_abs, worst_ratio = max(worst_abs, float(err.max())), max(worst_ratio, float((err / bound).max()))
        ref.grad = torch.from_numpy(g.copy())
        opt.step()
        differ = float((ref.detach().numpy().view(np.uint32) != p32.view(np.uint32)).mean())
    print(f"adamw kernel model vs torch float64 after 3 steps: max |dp| = {worst_abs:.3e}, worst err/bound = "
          f"{worst_ratio:.3f}; bit patterns differing from torch fp32 AdamW at step 3: {differ:.2f}")
    assert worst_ratio <= 1.0


def test_l1_restatement_is_the_oracle_projection():
    for kk in (1, 3, 50, 128):
        x = torch.from_numpy(R.l1_gauss_rows(kk, 0.03, kk)).double()
        ref = O.project_onto_l1_ball(x, R.R_GAUSS).numpy()
        got = R.l1ball_fp64(x.numpy(), R.R_GAUSS)
        assert np.abs(got["out"] - ref).max() <= 1e-15
        # the grid model is the float32 rounding of the same projection
        xg = R.l1_grid_rows(kk, 257, 0)
        ref = O.project_onto_l1_ball(torch.from_numpy(xg).double(), R.R_GRID).numpy()
        assert np.abs(R.l1ball_fp64(xg, R.R_GRID, R.Q)["out"] - ref).max() <= 2 * U * R.R_GRID * 4


def test_atom_restatements_are_constraint_dict():
    g = torch.Generator().manual_seed(1)
    d = torch.randn(3, 6, 7, 5, generator=g, dtype=torch.float64) * 0.2
    d[..., 0] *= 0.01
    assert np.abs(R.atom_scale_fp64(d, False) - O.constraint_dict(d, "l2ball").numpy()).max() <= 1e-15
    assert np.abs(R.atom_scale_fp64(d, True) - O.constraint_dict(d, "l2sphere").numpy()).max() <= 1e-14
    assert np.abs(R.atom_l1ball_fp64(d.numpy(), 1.0)["out"] - O.constraint_dict(d, "l1ball").numpy()).max() <= 1e-15
    half = R.atom_scale_fp64(d, False, 0.5)
    nrm = np.sqrt((half.reshape(-1, 5) ** 2).sum(axis=0))
    assert nrm.max() <= 0.5 + 1e-12 and np.allclose(half[..., 0], d[..., 0].numpy())
    x = torch.randn(40, 9, generator=g, dtype=torch.float64)
    ref = x * (0.7 / x.norm(dim=1, keepdim=True).clamp(min=0.7))
    assert np.abs(R.l2ball_fp64(x, 0.7) - ref.numpy()).max() <= 1e-15


def test_ista_metrics_inverse_and_fp8_restatements():
    g = torch.Generator().manual_seed(2)
    v, gr = torch.randn(999, generator=g, dtype=torch.float64), torch.randn(999, generator=g, dtype=torch.float64)
    assert np.array_equal(R.ista_fp64(v, gr, 0.1, 0.3), O.softshrink(v - 0.1 * gr, 0.3).numpy())
    assert np.array_equal(R.ista_fp64(v, None, 0.1, 0.3), torch.nn.Softshrink(0.3)(v).numpy())
    adv, x = R.metrics_operands(63, torch.float32)
    se, sn = R.image_metrics_fp64(adv, x)
    assert np.array_equal(se, ((adv - x).double() ** 2).sum(1).numpy()) and np.array_equal(sn, (x.double() ** 2).sum(1).numpy())
    for kk in (1, 2, 3, 4, 5, 7, 64, 65, 127, 128):
        a, inv = R.spd_family(kk)
        assert np.abs(a).max() <= 2 and np.abs(inv).max() <= kk and (inv != 0).all()
        assert np.abs(torch.linalg.inv(torch.from_numpy(a).double()).numpy() - inv).max() <= 1e-9 * kk
    d = torch.randn(64, generator=g) * 0.5
    ref = (d * 256.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)              # oracle.synth_fp8's quantiser
    assert np.array_equal(R.fp8_bytes(d), ref.view(torch.uint8).numpy())
    probe = R.fp8_probe_values()
    assert probe.size % 4 == 0 and set(R.fp8_bytes(probe).tolist()) >= set(range(0, 0x7f)) | set(range(0x81, 0xff))


# --------------------------------------------------------------------- every GPU row through the emulation of its kernel
@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", R.ADAMW_N)
def test_rows_adamw_flat(n, gdtype):
    R.check_adamw_flat(n, gdtype, run_flat())


def test_rows_adamw_dyn_and_fp8():
    R.check_adamw_flat(1025, torch.float32, run_flat(), dyn=True)
    for n in R.ADAMW_FP8_N:
        R.check_adamw_flat(n, torch.bfloat16 if n == 1024 else torch.float32, run_flat(), clamps=R.ADAMW_CLAMPS[:1], fp8=True)
    R.check_fp8(R.fp8_bytes)


@pytest.mark.parametrize("source", R.ROW_SOURCES)
@pytest.mark.parametrize("n,kk", R.ROWS_NK)
def test_rows_adamw_on_code_rows(n, kk, source):
    R.check_adamw_rows(n, kk, source, run_rows())


@pytest.mark.parametrize("nslabs", R.SLAB_COUNTS)
def test_rows_slab_sum(nslabs):
    R.check_slab(nslabs, run_pack(), run_rows())


@pytest.mark.parametrize("kk", R.L1_K)
def test_rows_l1_exact(kk):
    R.check_l1_exact(kk, run_l1())


def test_rows_l1_gauss():
    worst = max(R.check_l1_gauss(kk, run_l1()) for kk in R.L1_GAUSS_K)
    print(f"l1 gaussian leg, emulation: worst err/bound = {worst:.3f}")
    assert worst <= 1.0


def test_rows_l2():
    for kk in R.L2_K:
        R.check_l2_exact(kk, R.emu_l2ball)
    worst = max(R.check_l2_gauss(kk, R.emu_l2ball) for kk in R.L2_K)
    print(f"l2 gaussian leg, emulation: worst err/bound = {worst:.3f}")


def test_rows_atom_norms_and_scale():
    for p, kk in R.ATOM_SHAPES:
        R.check_atom_exact(p, kk, run_atom())
    print(f"atom gaussian leg, emulation: worst err/bound = {R.check_atom_gauss(run_atom()):.3f}")


def test_rows_atom_l1():
    for shape in R.ATOM_L1_SHAPES:
        R.check_atom_l1_exact(shape, R.emu_atom_l1)


def test_rows_ista():
    for n in R.ISTA_N:
        R.check_ista_exact(n, R.emu_ista)
        print(f"ista gaussian leg n={n}, emulation: worst err/bound = {R.check_ista_gauss(n, R.emu_ista):.3f}")


def test_rows_spd_inverse():
    for kk in R.SPD_K:
        R.check_spd(kk, R.emu_spd_inverse)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_rows_image_metrics(dtype):
    for p in R.METRIC_P:
        R.check_metrics_exact(p, dtype, run_metrics())


# ---------------------------------------------------------------------------------------------------------------- mutants
FLAT = lambda mutant: (lambda: R.check_adamw_flat(1023, torch.float32, run_flat(mutant)))       # noqa: E731
MUTANTS = {
    "tie-break dropped": lambda: R.check_l1_exact(50, run_l1("no_tiebreak")),
    "rho taken as min": lambda: R.check_l1_exact(50, run_l1("rho_min")),
    "theta divided by K": lambda: R.check_l1_exact(50, run_l1("theta_over_k")),
    "sign lost (l1)": lambda: R.check_l1_exact(3, run_l1("sign_lost")),
    "sign lost (atom l1)": lambda: R.check_atom_l1_exact((3, 1, 5, 2), lambda d, r: R.emu_atom_l1(d, r, "sign_lost")),
    "sign lost (ista)": lambda: R.check_ista_exact(37 * 50, lambda v, g, st, lam: R.emu_ista(v, g, st, lam, "sign_lost")),
    "eps inside the square root": FLAT("eps_in_sqrt"),
    "bc2_sqrt omitted": FLAT("no_bc2"),
    "decay applied after the step": FLAT("decay_after"),
    "torch's double-rounded 1 - b2": FLAT("torch_weights"),
    "n % 4 tail skipped": FLAT("tail_skipped"),
    "delta taken before the clamp": FLAT("delta_before_clamp"),
    "AdamW mutant on code rows": lambda: R.check_adamw_rows(67, 65, "pos", run_rows("torch_weights")),
    "max(n, 1) in sphere mode": lambda: R.check_atom_exact(300, 17, run_atom("max_in_sphere")),
    "slab tail weight missing (pack_codes)": lambda: R.check_slab(33, run_pack("no_tail_weight"), run_rows()),
    "slab tail weight missing (adamw)": lambda: R.check_slab(65, run_pack(), run_rows("no_tail_weight")),
    "fp8 scale 128": lambda: R.check_fp8(lambda x: R.fp8_bytes(x, 128.0)),
    "fp8 scale 128 (fused copy)": lambda: R.check_adamw_flat(1024, torch.float32, run_flat("fp8_scale_128"),
                                                              clamps=R.ADAMW_CLAMPS[:1], fp8=True),
    "l2 row tail (N % 4) skipped": lambda: R.check_l2_exact(65, lambda x, r: R.emu_l2ball(x, r, "row_tail_skipped")),
    "inverse: last pivot column kept": lambda: R.check_spd(5, lambda a: R.emu_spd_inverse(a, "pivot_column_kept")),
    "metrics: elements past the last whole vector dropped": lambda: R.check_metrics_exact(63, torch.float32,
                                                                                          run_metrics("vector_tail_dropped")),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_exact_legs_reject_mutant(name):
    with pytest.raises(AssertionError):
        MUTANTS[name]()


def test_michelot_ge_is_not_a_mutant():
    """Keeping the entries with |x| == theta active (`>=` for `>`) leaves theta where it is: (s + theta - r) / (n + 1) =
    theta when (s - r) / n = theta.  The outputs are the same bits, so this variant is not in MUTANTS."""
    for shape in R.ATOM_L1_SHAPES[:3]:
        d = R.atom_l1_grid(shape)
        R.assert_bits_equal(R.emu_atom_l1(d, 1.0, "michelot_ge"), R.emu_atom_l1(d, 1.0), f"michelot >= {shape}")


# --------------------------------------------------------------------------------------------------------------- vacuity
@pytest.mark.parametrize("kk", R.L1_K)
def test_l1_rows_contain_their_cases(kk):
    sets = [R.l1ball_fp64(R.l1_grid_rows(kk, n, 0), R.R_GRID, R.Q) for n in R.L1_N]
    big = sets[-1]
    frac = float(big["projected"].mean())
    ties = float(big["has_tie"].sum()) / max(1, int(big["projected"].sum()))
    print(f"K={kk}: projected {frac:.2f}, ties among projected rows {ties:.2f}")
    assert frac >= 0.5
    if kk >= 10:
        assert ties >= 0.10
    nz = (R.l1_grid_rows(kk, R.L1_N[-1], 0) != 0).sum(axis=1)
    allrows = lambda key: np.concatenate([s[key] for s in sets])                 # noqa: E731
    assert allrows("on_boundary").any() and (allrows("S") == 0).any() and (~allrows("projected") & (allrows("S") > 0)).any()
    assert (nz == 1).any()
    assert ((big["rho"] == 1) & big["projected"]).any() and ((big["rho"] == kk) & big["projected"]).any()
    if kk in R.L1_GAUSS_K:                                         # gaussian leg: every scale has rows on both sides of r
        for si, scale in enumerate(R.l1_gauss_scales(kk)):
            ref = R.l1ball_fp64(R.l1_gauss_rows(kk, scale, 100 * kk + si), R.R_GAUSS)
            assert ref["projected"].any() and (scale > 0.5 or (~ref["projected"]).any())


def test_other_row_sets_contain_their_cases():
    for kk in R.L2_K:                                              # l2: inside, outside and zero rows
        x = R.l2_grid_rows(kk, 258)
        nrm = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
        assert (nrm == 0).any() and ((nrm > 0) & (nrm < R.L2_R)).any() and ((nrm > R.L2_R).any() or kk == 1)
    assert (np.abs(R.l2_grid_rows(1, 258)) > R.L2_R).any()
    for p, kk in R.ATOM_SHAPES:                                    # atoms: one below norm 1, the others above (P >= 8)
        n = R.atom_norms_fp64(R.atom_grid(p, kk))
        assert (n > 0).all() and n[0] < 1 and (p < 8 or kk == 1 or (n[1:] > 1).all())
    seen = dict(inside=False, boundary=False, rho1=False, tie=False)
    for shape in R.ATOM_L1_SHAPES:
        ref = R.atom_l1ball_fp64(R.atom_l1_grid(shape), 1.0, R.Q)
        seen["inside"] |= bool((~ref["projected"]).any())
        seen["boundary"] |= bool(ref["on_boundary"].any())
        seen["rho1"] |= bool(((ref["rho"] == 1) & ref["projected"] & (shape[1] * shape[2] > 1)).any())
        seen["tie"] |= bool(ref["has_tie"].any())
        assert ref["projected"].any()
    assert all(seen.values()), seen
    for n in R.ISTA_N:                                             # ista: all three branches and both boundaries
        rng = np.random.default_rng(n)
        v = (rng.integers(-1024, 1025, size=n) * 2.0 ** -10)
        assert (v > 0.125).any() and (v < -0.125).any() and (np.abs(v) <= 0.125).any()
    p, gs = R.adamw_operands(1023, torch.float32)                  # AdamW: clamped elements on both sides, exact zeros
    q, _, _, _, _ = R.adamw_elem_f32(p, gs[0].numpy(), np.zeros_like(p), np.zeros_like(p), R.adamw_hyper(0.01, 1), -0.5, 0.5)
    assert (q == F32(-0.5)).any() and (q == F32(0.5)).any() and (np.abs(q) < 0.5).any() and (gs[0] == 0).any()
