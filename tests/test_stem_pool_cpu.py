"""CPU: the restatement of the stem's pooling pair (tests/stem_pool_reference.py) against torch, against its own fp32
emulation of the backward kernel, and against thirteen mutants; the exact-sum premise cap of the gaussian leg; the Python
refusal of a batch the stem convolutions cannot launch."""
import os

import pytest
import torch
import torch.nn.functional as F

import stem_pool_reference as P
from classifier_reference import BF16, F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("exact", "gaussian")
POOL_ROWS = [r for r in P.SMALL_ROWS if r.cls in P.Y_CLASSES]


def _id(r):
    return r.name


@pytest.fixture(scope="module")
def cases():
    """Per (row, leg) of the small rows: operands, (p, idx) and the backward reference.  Computed once, never modified."""
    out = {}
    for r in P.SMALL_ROWS:
        for leg in LEGS:
            o = P.operands(r, leg)
            p, idx = P.forward_of(r, o)
            out[r, leg] = (o, p, idx, P.pool_bwd(o["g"], idx, p, o["scale"], r.shape[1], r.shape[2]))
    return out


def test_rows_cover_the_contract():
    assert {r.shape for r in P.ROWS} == set(P.SHAPES) | {P.NEAR_TIE_SHAPE}
    for s in P.EVERY_CLASS_AT:
        assert {r.cls for r in P.ROWS if r.shape == s} >= set(P.Y_CLASSES)
    for s in P.SHAPES:
        want = {"relu"} if s == P.PRODUCT_SHAPE else {"relu", "ints"}
        assert {r.cls for r in P.ROWS if r.shape == s} >= want
    assert P.Row(*P.ZERO_SCALE_ROW) in P.ROWS
    assert float(P.operands(P.Row(*P.ZERO_SCALE_ROW), "exact")["scale"][P.ZERO_SCALE_CHANNEL]) == 0.0
    for s in P.EVERY_CLASS_AT:
        two_nans, only_ninf = P.special_windows(P.operands(P.Row(s, "special"), "exact")["y"])
        assert two_nans >= 1 and only_ninf >= 1, (s, two_nans, only_ninf)
    y = P.operands(P.Row((3, 17, 23, 64), "relu"), "exact")["y"]
    p, _ = P.maxpool_fwd(y)
    share = float((p == 0).double().mean())
    assert 0.001 < share, share                                          # windows that hold only +0 exist
    syn = P.operands(P.Row((3, 17, 23, 64), "synthetic"), "exact")
    pv = syn["p"].float()
    assert bool(torch.isnan(pv).any()) and bool((pv == 1).any()) and bool((pv == -1).any())
    assert bool(((pv == 0) & torch.signbit(pv)).any()) and bool(((pv == 0) & ~torch.signbit(pv)).any())


@pytest.mark.parametrize("row", [r for r in P.ROWS if r.cls in P.Y_CLASSES], ids=_id)
def test_maxpool_restatement_equals_torch(row):
    """Values and indices of torch.nn.functional.max_pool2d(3, 2, 1) on the CPU in fp32, every class at every shape: the
    header's claim of torch's rule, the two-NaN window and the all -inf window included."""
    B, OH, OW, C = row.shape
    y = P.operands(row, "exact")["y"]
    p, idx = P.maxpool_fwd(y)
    t = y.float().permute(0, 3, 1, 2).contiguous()
    tp, ti = F.max_pool2d(t, 3, 2, 1, return_indices=True)
    tp, ti = tp.permute(0, 2, 3, 1), ti.permute(0, 2, 3, 1)              # flat plane index ih * OW + iw
    ph = torch.arange(P.pooled(OH)).view(1, -1, 1, 1)
    pw = torch.arange(P.pooled(OW)).view(1, 1, -1, 1)
    tk = ((ti // OW) - (2 * ph - 1)) * 3 + (ti % OW) - (2 * pw - 1)
    P.same_selection(row.name + " against torch", p, idx, tp, tk.to(torch.uint8), OH, OW)
    if row.cls == "const":
        assert bool((p.view(torch.int32) == torch.tensor(P.CONST_VALUE).view(torch.int32)).all())
        want = torch.zeros(P.pooled(OH), P.pooled(OW), dtype=torch.uint8)
        # the first tap in range: (1, 0) = 3 in the top row (row -1 is padding), (0, 1) = 1 in the left column, (1, 1) = 4 in
        # the corner, (0, 0) = 0 inside; torch gives the same
        want[0, :], want[:, 0], want[0, 0] = 3, 1, 4
        assert torch.equal(idx, want.view(1, *want.shape, 1).expand_as(idx))
    if row.cls == "special":
        assert int(idx[0, 2, 2, 1]) == 5 and bool(torch.isnan(p[0, 2, 2, 1]))          # the LAST NaN of the window
        assert int(idx[0, 0, 0, 0]) == 4 and float(p[0, 0, 0, 0]) == float("-inf")      # the first tap in range


@pytest.mark.parametrize("row", [r for r in POOL_ROWS if r.cls != "special"], ids=_id)
def test_pool_bwd_restatement_equals_torch_autograd(row, cases):
    """The fp64 sum times the scale, before any rounding, is torch autograd of max_pool2d followed by the mask [y > 0] and
    the scale in fp64.  The `special` rows are left to the selection test above: their routing is the idx compared there."""
    B, OH, OW, C = row.shape
    for leg in LEGS:
        o, p, idx, ref = cases[row, leg]
        t = o["y"].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        F.max_pool2d(t, 3, 2, 1).backward(o["g"].double().permute(0, 3, 1, 2))
        want = (t.grad * (t.detach() > 0)).permute(0, 2, 3, 1) * o["scale"].double()
        assert torch.equal(ref.sum * o["scale"].double() + 0.0, want + 0.0), (row.name, leg)


@pytest.mark.parametrize("row", P.SMALL_ROWS, ids=_id)
def test_emulation_equals_reference(row, cases):
    """The gather form in fp32 equals the scatter form in fp64 bit for bit, on both legs."""
    B, OH, OW, C = row.shape
    for leg in LEGS:
        o, p, idx, ref = cases[row, leg]
        rep = P.compare_gy(f"{row.name} [{leg}]", P.emulate_pool_bwd(o["g"], idx, p, o["scale"], OH, OW), ref, leg == "exact")
        assert rep.off_premise == 0 or leg == "gaussian"


def test_premise_cap_holds_on_every_gaussian_row(cases):
    """At most 1e-4 of a row's elements may be off the exact-sum premise; asserted here on the reference alone, the product's
    grid included, so the GPU test cannot hide behind the bound."""
    counts = {}
    for r in P.ROWS:
        if (r, "gaussian") in cases:
            ref = cases[r, "gaussian"][3]
        else:
            o = P.operands(r, "gaussian")
            p, idx = P.forward_of(r, o)
            ref = P.pool_bwd(o["g"], idx, p, o["scale"], r.shape[1], r.shape[2])
        off = int((~ref.exact_sum).sum())
        counts[r.name] = off
        multi = float((ref.n > 1).double().mean())
        assert int(ref.n.max()) <= 4
        assert off <= P.PREMISE_CAP * ref.sum.numel(), (r.name, off, ref.sum.numel())
        print(f"{r.name}: {off} of {ref.sum.numel()} elements off the premise; {100 * multi:.1f} % receive more than one gradient")
    for r in P.ROWS:
        ref = cases[r, "exact"][3] if (r, "exact") in cases else None
        if ref is not None:
            assert bool(ref.exact_sum.all()), r.name


def test_exact_leg_rounds_and_ties(cases):
    """The exact leg's final rounding really rounds, and exact ties occur."""
    r = P.Row((3, 17, 23, 64), "relu")
    nz, rounded, tie = P.rounding_stats(cases[r, "exact"][3])
    print(f"{r.name}: non-zero {100 * nz:.1f} %, really rounded {100 * rounded:.2f} %, exact ties {100 * tie:.2f} %")
    assert rounded > 0.01 and tie > 0.001, (rounded, tie)


# ------------------------------------------------------------------------------------------------------------ mutants
# Mutants that no bit-exact comparison of these rows can see, with the reason.  Empty: every mutant is killed.
PINNED = {}


def _killers_fwd(mutant, cases):
    out = []
    for r in POOL_ROWS:
        o, p, idx, _ = cases[r, "exact"]
        try:
            mp, mi = P.maxpool_fwd(o["y"], (mutant,))
            P.same_selection(r.name, mp, mi, p, idx, r.shape[1], r.shape[2])
        except AssertionError:
            out.append(r.name)
    return out


def _killers_bwd(mutant, cases):
    out = []
    for r in P.SMALL_ROWS:
        for leg in LEGS:
            o, p, idx, ref = cases[r, leg]
            try:
                P.compare_gy(r.name, P.emulate_pool_bwd(o["g"], idx, p, o["scale"], r.shape[1], r.shape[2], (mutant,)), ref,
                             leg == "exact")
            except AssertionError:
                out.append(f"{r.name} [{leg}]")
    return out


# the row each mutant must be killed by (others may kill it too): the edge the mutant is about
KILLED_BY = {
    "ge": "3x17x23x64-ints", "start_at_zero": "3x17x23x64-negative", "nan_loses": "3x17x23x64-special",
    "idx_transposed": "2x16x16x64-relu", "origin_2ph": "2x2x2x8-relu", "next_image": "3x17x23x64-negative",
    "mask_ge": "3x17x23x64-relu [exact]", "no_mask": "3x17x23x64-synthetic [exact]", "first_window_only": "3x17x23x64-ints [exact]",
    "clamped_window": "2x16x16x64-ints [exact]", "neighbour_scale": "2x5x4x72-relu [exact]", "trunc": "3x17x23x64-relu [exact]",
    "scale_each_term": "1x3x3x512-near_tie [exact]",
}


@pytest.mark.parametrize("mutant", P.MUTANTS_FWD + P.MUTANTS_BWD)
def test_every_mutant_fails_a_bit_exact_comparison(mutant, cases):
    killers = (_killers_fwd if mutant in P.MUTANTS_FWD else _killers_bwd)(mutant, cases)
    print(mutant, "killed by", len(killers), "comparisons:", ", ".join(killers[:6]))
    if mutant in PINNED:
        assert not killers, (mutant, killers)
    else:
        assert KILLED_BY[mutant] in killers, f"mutant {mutant}: row {KILLED_BY[mutant]} does not kill it; killed by {killers}"


def test_mutant_lists_are_the_thirteen():
    assert len(P.MUTANTS_FWD) == 6 and len(P.MUTANTS_BWD) == 7 and set(KILLED_BY) == set(P.MUTANTS_FWD + P.MUTANTS_BWD)


# ---------------------------------------------------------------------------------------------------- library, header
def test_header_states_the_pooling_arithmetic_and_the_batch_limit():
    header = open(os.path.join(ROOT, "include", "adil_hip.h")).read()
    for words in ("1 <= B <= 65535", "padding taps are ABSENT", "LAST NaN", "ascending (ph, pw) order", "p > 0 BY VALUE",
                  "no sign of zero is promised"):
        assert words in header, words


def test_stem_function_refuses_a_batch_beyond_the_grid_limit(monkeypatch):
    """ValueError before the library is called (the library would answer ADIL_EINVAL)."""
    from dl_attack_on_imagenet_amd import _lib, ops
    assert ops.STEM_MAX_BATCH == 65535

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    monkeypatch.setattr(_lib, "load", lambda *a, **k: NoCalls())
    monkeypatch.setattr(ops, "_dev", lambda t, *a, **k: t)
    x = torch.zeros(ops.STEM_MAX_BATCH + 1, 3, 2, 2)
    z = torch.zeros(1)
    with pytest.raises(ValueError, match="65535"):
        ops.StemFunction.apply(x, z, z, z, z, (0.0,) * 3, (1.0,) * 3)
