"""tests/contract_reference.py checked without a GPU:

* the restatements against plain torch float64 and the oracle;
* every row of tests/test_gpu_contract_exact.py run through the numpy emulation of its kernel, through the very check
  function the GPU file uses: the rows are known to pass for a correct kernel before anyone has a GPU (rows above
  B P K = 2^27 would be listed in OVER_CAP; there are none in the synthesis and z-step families);
* vacuity, on the reference alone: the rows contain what they are meant to contain (inexact and tied bf16 roundings,
  binding clamps, a non-zero m plane on the mid grid and l plane on the wide grid, gz == 0 elements);
* the exact legs reject every mutant (a deliberately wrong kernel variant); a mutant that turns out to be equivalent is
  pinned as equivalent.
"""
import numpy as np
import pytest
import torch

import contract_reference as C
import update_reference as U
from contract_reference import F32
from oracle import adil_oracle as O
from test_gpu_routes import ROUTES

CAP = 2 ** 27
OVER_CAP = []


# ------------------------------------------------------------------------------------------------- emulation "wrappers"
def run_synth(mutant=None):
    return lambda c: C.emu_synth(c, mutant)


def run_store(mutant=None):
    def run(store, index, c):
        out = C.emu_synth(c, mutant)
        out["gathered"] = C.emu_synth(c)["out"] if c.stream == "f32" else None
        return out
    return run


def run_zstep(mutant=None, codes=False):
    def run(z, m, s, dpt, gv, h, lo, hi, dyn, off):
        if dyn is not None:                                          # the device scalars win over the host's
            h = h[:4] + tuple(dyn)
        return C.emu_zstep(z, m, s, dpt, gv, h, lo, hi, mutant, codes)
    return run


UNALIGNED = [C.SynthRow("bf16" if r.dtype == torch.bfloat16 else "f32", r.shape[4], r.shape[1] * r.shape[2] * r.shape[3],
                        r.shape[0], r.offset) for r in ROUTES if r.entry == "synth" and r.offset]


# ------------------------------------------------------------------------------------------ restatements against torch
def test_number_formats():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0000001, 2.0 ** -130, 0.0], F32)      # 1 + 2^-8: a tie, to even
    assert np.array_equal(C.rne_bf16(x)[:3], np.array([1.0, 1.0, 1.015625], F32))
    assert np.array_equal(C.trunc_bf16(x)[:3], np.array([1.0, 1.0, 1.0078125], F32))
    rng = np.random.default_rng(0)
    a = (rng.standard_normal(4096) * 2.0 ** rng.integers(-20, 20, 4096)).astype(F32)
    p = C.split3(a)
    for piece in p.values():
        assert np.array_equal(C.rne_bf16(piece), piece)
    assert np.array_equal(p["h"].astype(np.float64) + p["m"] + p["l"], a.astype(np.float64)), "three bf16 pieces hold 24 bits"
    assert np.array_equal(C.e4m3(np.array([449.0, 600.0, -600.0, 17.0, 19.0, 8.5], F32)), np.array([448, 448, -448, 16, 20, 8], F32))
    assert np.isnan(C.e4m3(np.array([600.0], F32), saturate=False)).all()
    assert C.sig_bits(np.array([0.0, 1.0, 3.0, 0.75, 257.0, 1.0 + 2.0 ** -23])).tolist() == [0, 1, 2, 2, 9, 24]
    assert float(C.low_quantum(np.array([[0.75, 0.0], [4.0, 0.0]]), 0)[0]) == 0.25


def test_synth_restatement_is_the_oracle_in_float64():
    r = C.SynthRow("f32", 50, 432, 70)
    c = next(iter(C.gauss_cases(r)))
    ref, s = C.ref_synth(c)
    x, d, v = (torch.from_numpy(a).double() for a in (c.x, c.d, c.v))
    want = O.synth(x, d.reshape(3, 12, 12, 50), v)
    assert float((torch.from_numpy(ref) - want).abs().max()) <= 1e-14
    clamped = c._replace(delta=0.01, pixel=True)
    dv = (v @ d.t()).clamp(-float(F32(0.01)), float(F32(0.01)))
    assert float((torch.from_numpy(C.ref_synth(clamped)[0]) - (x + dv).clamp(0, 1)).abs().max()) <= 1e-15
    bf = c._replace(stream="bf16")
    want = x + v.float().bfloat16().double() @ d.float().bfloat16().double().t()
    assert float((torch.from_numpy(C.ref_synth(bf)[0]) - want).abs().max()) <= 1e-14
    # fp8: the oracle's restatement (it rounds its result to fp32)
    f8 = next(iter(C.gauss_cases(r, fp8=True)))
    want = O.synth_fp8(torch.from_numpy(f8.x), torch.from_numpy(f8.d).reshape(3, 12, 12, 50), torch.from_numpy(f8.v), f8.fp8)
    assert float((torch.from_numpy(C.ref_synth(f8)[0]) - want.double()).abs().max()) <= 2e-7


def test_zstep_restatement_is_the_oracle_sequence():
    """gz = gv D_dagger, AdamW, clamp, max |dz| of the emulation against the oracle's float64 AdamWState."""
    rng = np.random.default_rng(1)
    b, p, k = 5, 64, 7
    dpt = (0.1 * rng.standard_normal((p, k))).astype(F32)
    gv = rng.standard_normal((b, k)).astype(F32)
    z = (0.01 * rng.standard_normal((b, p))).astype(F32)
    zr = torch.from_numpy(z).double()
    st = O.AdamWState(zr, C.Z_LR)
    m, s = np.zeros_like(z), np.zeros_like(z)
    for it in range(3):
        got = C.emu_zstep(z, m, s, dpt, gv, U.adamw_hyper(C.Z_LR, it + 1), -C.Z_EPS, C.Z_EPS, codes=True)
        prev = zr.clone()
        st.step(zr, torch.from_numpy(gv).double() @ torch.from_numpy(dpt).double().t())
        zr.clamp_(-C.Z_EPS, C.Z_EPS)
        assert float((torch.from_numpy(got["z"]).double() - zr).abs().max()) <= 5e-5
        assert abs(float(got["delta"]) - float((zr - prev).abs().max())) <= 5e-5
        ref = got["z"].astype(np.float64) @ dpt.astype(np.float64)
        assert np.abs(got["codes"] - ref).max() <= float(C.codes_bound(np.abs(got["z"]) @ np.abs(dpt), p).max())
        z, m, s = got["z"], got["m"], got["s"]


# ------------------------------------------------------------------------------------- the GPU rows through the emulation
def test_no_row_is_over_the_cap():
    sizes = [r.b * r.p * r.k for r in C.SYNTH_ROWS + UNALIGNED + C.FP8_ROWS + C.SYNTH_GAUSS_ROWS + C.STORE_ROWS + C.Z_ROWS + C.ZC_ROWS]
    assert OVER_CAP == [] and max(sizes) <= CAP


@pytest.mark.parametrize("r", C.SYNTH_ROWS + UNALIGNED, ids=C.synth_row_id)
def test_synth_rows_pass_the_emulation(r):
    for grid in C.SYNTH_GRIDS[r.stream]:
        C.check_synth_exact(r, grid, run_synth())


@pytest.mark.parametrize("r", C.FP8_ROWS, ids=C.synth_row_id)
def test_fp8_rows_pass_the_emulation(r):
    for kind in C.FP8_KINDS:
        C.check_synth_fp8(r, kind, run_synth())


def test_gauss_and_store_rows_pass_the_emulation():
    for r in C.SYNTH_GAUSS_ROWS:
        print(f"{C.synth_row_id(r)} gauss: emulation worst err/bound = {C.check_synth_gauss(r, run_synth()):.3f}, "
              f"fp8 {C.check_synth_gauss(r, run_synth(), fp8=True):.5f}")
    for r in C.STORE_ROWS:
        print(f"{C.synth_row_id(r)} store: emulation worst err/bound = {C.check_synth_store(r, run_store()):.3f}")


@pytest.mark.parametrize("r", C.Z_ROWS, ids=C.zrow_id)
def test_zstep_rows_pass_the_emulation(r):
    for grid in ("narrow", "mid"):
        C.check_zstep(r, grid, run_zstep())


@pytest.mark.parametrize("r", C.ZC_ROWS, ids=C.zrow_id)
def test_zstep_codes_rows_pass_the_emulation(r):
    worst = C.check_zstep_codes(r, run_zstep(codes=True), run_zstep())
    print(f"{C.zrow_id(r)} gaussian codes: emulation worst err/bound = {worst:.4f}")


# ------------------------------------------------------------------------------------------------------------------ vacuity
def test_synth_rows_contain_what_they_are_for():
    """Shares over the reference alone, per stream type and grid: bf16 roundings that are inexact / ties, elements where
    the delta clamp binds (perturbation below, equal to and above delta all occur) and where the pixel clamp binds at
    either end; the m plane of the mid grid and the l plane of the wide grid are not empty."""
    for grid in ("narrow", "mid"):
        inexact = ties = total = 0
        below = equal = above = under0 = over1 = n = 0
        for r in (r for r in C.SYNTH_ROWS if r.stream == "bf16"):
            for c in C.synth_cases(r, grid):
                ref, _ = C.ref_synth(c)
                r32 = ref.astype(F32)
                rounded = C.rne_bf16(r32)
                inexact += int((rounded != r32).sum())
                lo = C.trunc_bf16(r32)                                                # the bf16 neighbour towards zero
                up = (lo.view(np.uint32) + np.uint32(0x10000)).view(F32)             # the bf16 neighbour away from zero
                ties += int(((r32 != lo) & ((r32.astype(np.float64) - lo) == (up.astype(np.float64) - r32))).sum())
                total += ref.size
                if c.delta >= 0 and not c.pixel:
                    dv = C.synth_operands64(c)[0] @ C.synth_operands64(c)[1].T
                    below += int((np.abs(dv) < c.delta).sum())
                    equal += int((np.abs(dv) == c.delta).sum())
                    above += int((np.abs(dv) > c.delta).sum())
                if c.pixel and c.delta < 0:
                    raw, _ = C.ref_synth(c._replace(pixel=False))
                    under0 += int((raw < 0).sum())
                    over1 += int((raw > 1).sum())
                    n += raw.size
        print(f"{grid}: bf16 store inexact {inexact / total:.3f}, ties {ties / total:.4f}; delta clamp: |VD^T| below "
              f"{below}, equal {equal}, above {above}; pixel clamp binds below 0 {under0 / n:.3f}, above 1 {over1 / n:.3f}")
        assert inexact and ties and below and above and under0 and over1
        if grid == "narrow":
            assert equal
    r = C.SYNTH_ROWS[3]
    d, v = C.mid_dv(np.random.default_rng(0), r.p, r.k, r.b)
    for a in (d, v):
        p = C.split3(a)
        assert p["m"].any() and not p["l"].any()
    bits = C.sig_bits(np.concatenate([d.ravel(), v.ravel()]))
    assert 9 in bits and 16 in bits and bits.max() == 16
    halfway = (C.rne_bf16(d) != C.trunc_bf16(d)) & (C.sig_bits(d) == 9)
    assert halfway.any(), "no operand exactly halfway between two bf16 numbers"
    for wide in ("v", "d"):
        d, v = C.wide_dv(np.random.default_rng(0), r.p, r.k, r.b, wide)
        w = C.split3(v if wide == "v" else d)
        share = float((w["l"] != 0).mean())
        print(f"wide {wide}: l plane non-zero on {share:.3f} of the operand")
        assert share > 0.5 and w["m"].any() and (C.sig_bits(v if wide == "v" else d) == 24).all()


def test_zstep_rows_contain_what_they_are_for():
    for r in C.Z_ROWS:
        for grid in ("narrow", "mid"):
            v = C.zstep_vacuity(r, grid)
            print(f"{C.zrow_id(r)} {grid}: gz == 0 on {v['gz_zero']:.3f}, clamp binds on {v['clamp_binds']:.3f}")
            assert v["gz_zero"] >= 0.3 and v["clamp_binds"] > 0


# ------------------------------------------------------------------------------------------------------------------ mutants
def rejected(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


F32_ROW, BF16_ROW = C.SynthRow("f32", 50, 432, 70), C.SynthRow("bf16", 50, 432, 70)
# mutant -> (row, grid) of an exact leg that must reject it
SYNTH_MUTANTS = {
    "drop_hh": (F32_ROW, "narrow"), "drop_hm": (F32_ROW, "mid"), "drop_mh": (F32_ROW, "mid"), "drop_mm": (F32_ROW, "mid"),
    "drop_lh": (F32_ROW, "wide_v"), "drop_hl": (F32_ROW, "wide_d"), "swap_ml": (F32_ROW, "mid"),
    "trunc_operand": (BF16_ROW, "mid"), "trunc_out": (BF16_ROW, "narrow"), "delta_after_x": (F32_ROW, "narrow"),
    "pixel_before_delta": (F32_ROW, "narrow"), "x_twice": (F32_ROW, "narrow"), "skip_last_group": (F32_ROW, "narrow"),
    "pad_not_zeroed": (F32_ROW, "narrow"), "row_ge_B_stored": (F32_ROW, "narrow"),
}


@pytest.mark.parametrize("mutant", sorted(SYNTH_MUTANTS))
def test_synth_exact_legs_reject(mutant):
    r, grid = SYNTH_MUTANTS[mutant]
    assert not rejected(C.check_synth_exact, r, grid, run_synth())
    assert rejected(C.check_synth_exact, r, grid, run_synth(mutant)), f"{mutant} passes {grid}"


def test_only_the_wide_grids_see_the_l_plane_and_swap_ml_is_equivalent_there():
    """a.l b.h is needed by wide V alone, a.h b.l by wide D alone.  Exchanging the m and l planes of the dictionary image
    turns a.m b.m into a.m b.l (the mid grid rejects that) but keeps the SET {a.h b.m, a.h b.l}: with a one-hot partner
    (a.m = a.l = 0) the wide grids cannot tell, pinned here as equivalent."""
    for mutant in ("drop_lh", "drop_hl"):
        for grid in ("narrow", "mid"):
            assert not rejected(C.check_synth_exact, F32_ROW, grid, run_synth(mutant)), (mutant, grid)
    for grid in ("wide_v", "wide_d"):
        assert not rejected(C.check_synth_exact, F32_ROW, grid, run_synth("swap_ml")), grid


def test_operand_truncation_is_not_a_mutant_on_fp32_streams():
    """Truncating instead of rounding inside the three-way split still leaves h + m + l == x for every fp32 x (three
    8-bit pieces hold 24 bits either way), so on the exact legs the products are the same: equivalent, pinned."""
    for grid in C.SYNTH_GRIDS["f32"]:
        assert not rejected(C.check_synth_exact, F32_ROW, grid, run_synth("trunc_operand")), grid


@pytest.mark.parametrize("mutant", ["fp8_scale_128", "fp8_no_saturation", "skip_last_group", "x_twice"])
def test_fp8_legs_reject(mutant):
    r = C.FP8_ROWS[0]
    kind = "saturating" if mutant == "fp8_no_saturation" else "quantised"
    assert not rejected(C.check_synth_fp8, r, kind, run_synth())
    assert rejected(C.check_synth_fp8, r, kind, run_synth(mutant)), mutant


def test_store_row_rejects_a_wrong_table():
    """A byte table built as u * (1 / 255.f) (wrong in 126 of 256 entries, by one ulp) stays inside the float64 bound; it is
    the bitwise comparison with synth(gather_images(...)) that rejects it."""
    def run(store, index, c):
        out = C.emu_synth(c._replace(x=(store[index].astype(F32) * F32(1.0 / 255.0)).astype(F32)))
        out["gathered"] = C.emu_synth(c)["out"]
        return out
    assert not rejected(C.check_synth_store, C.STORE_ROWS[0], run_store())
    assert rejected(C.check_synth_store, C.STORE_ROWS[0], run)


Z_MUTANTS = ("drop_hh", "drop_hm", "drop_mh", "drop_mm", "swap_ml", "skip_last_group", "pad_not_zeroed", "delta_before_clamp")


@pytest.mark.parametrize("mutant", Z_MUTANTS)
def test_zstep_exact_legs_reject(mutant):
    r = C.ZRow(33, 768, 50)
    assert rejected(C.check_zstep, r, "narrow" if mutant in ("drop_hh", "delta_before_clamp") else "mid", run_zstep(mutant))


@pytest.mark.parametrize("mutant", ["codes_from_old_z", "drop_hh", "skip_last_group", "delta_before_clamp"])
def test_zstep_codes_legs_reject(mutant):
    r = C.ZRow(33, 768, 33)
    assert rejected(C.check_zstep_codes, r, run_zstep(mutant, codes=True), run_zstep())
