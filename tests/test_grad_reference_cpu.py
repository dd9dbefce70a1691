"""tests/grad_reference.py checked without a GPU:

* the restatements against plain torch float64 and the oracle (O.grad_dv, the autograd gradient of O.synth, O.gram_pinv);
* grad_plan against a hand-written table with a row per launcher branch; the exact rows of test_gpu_grad_exact.py reach
  every template instantiation launch_grad can launch (listed here by hand from csrc/adil_contract.hip) and walk at least
  two tiles per workgroup in every kernel that has a tile loop;
* every row of tests/test_gpu_grad_exact.py through the numpy emulation and the very check functions the GPU file uses
  (no row exceeds B P K = 2^27);
* the exact legs reject every mutant, each paired with the leg that must fail; equivalent mutants are pinned as such;
* vacuity on the reference alone.

Run time of the whole file: profiles/grad_exact.md.
"""
import itertools

import numpy as np
import pytest
import torch

import contract_reference as C
import grad_reference as G
from contract_reference import F32
from grad_reference import GradRow
from oracle import adil_oracle as O

CAP = 2 ** 27
NUM_CU = 256


def run_grad(mutant=None):
    def run(c, plan):
        res = G.emu_grad(c, NUM_CU, mutant)
        res["again"] = res
        return res
    return run


# ------------------------------------------------------------------------------------------ restatements against torch
def test_restatements_against_torch_and_oracle():
    rng = np.random.default_rng(1)
    b, p, k = 37, 3 * 4 * 5, 21
    g = rng.standard_normal((b, p)).astype(F32)
    d = rng.uniform(-1, 1, (p, k)).astype(F32)
    v = (0.02 * rng.standard_normal((b, k))).astype(F32)
    gd, sd, gv, sv = G.ref_grad(g, d, v, "f32")
    tg, td, tv = (torch.from_numpy(a).double() for a in (g, d, v))
    assert np.allclose(gd, (tg.t() @ tv).numpy(), rtol=1e-13, atol=0) and np.allclose(gv, (tg @ td).numpy(), rtol=1e-13, atol=0)
    od, ov = O.grad_dv(tg.reshape(b, 3, 4, 5), td.reshape(3, 4, 5, k), tv)
    assert np.allclose(gd, od.reshape(p, k).numpy(), rtol=1e-12, atol=1e-15) and np.allclose(gv, ov.numpy(), rtol=1e-12, atol=1e-15)
    # the gradient of the oracle's synthesis, by autograd
    dd, vv = td.reshape(3, 4, 5, k).clone().requires_grad_(), tv.clone().requires_grad_()
    O.synth(torch.zeros(b, 3, 4, 5, dtype=torch.float64), dd, vv).backward(tg.reshape(b, 3, 4, 5))
    assert np.allclose(gd, dd.grad.reshape(p, k).numpy(), rtol=1e-12, atol=1e-15) and np.allclose(gv, vv.grad.numpy(), rtol=1e-12, atol=1e-15)
    # bf16 streams multiply the rounded V and D
    gb = C.rne_bf16(g)
    gd, _, gv, _ = G.ref_grad(gb, d, v, "bf16")
    tb = torch.from_numpy(gb).double()
    assert np.allclose(gd, (tb.t() @ tv.float().bfloat16().double()).numpy(), rtol=1e-13, atol=0)
    assert np.allclose(gv, (tb @ td.float().bfloat16().double()).numpy(), rtol=1e-13, atol=0)
    init = rng.standard_normal((p, k)).astype(F32)
    assert np.allclose(G.ref_grad(g, d, v, "f32", init)[0], (tg.t() @ tv).numpy() + init, rtol=1e-13, atol=0)
    # Gram and D M^T
    dtd, _, _ = O.gram_pinv(td.reshape(3, 4, 5, k))
    assert np.allclose(G.ref_gram(d)[0], dtd.numpy(), rtol=1e-12, atol=1e-15)
    m = rng.standard_normal((k, k)).astype(F32)
    assert np.allclose(G.ref_rightmul(d, m)[0], (td @ torch.from_numpy(m).double().t()).numpy(), rtol=1e-13, atol=0)
    # D (DtD)^-1 through the restatement is the oracle's D_dagger, transposed
    _, inv, ddrg = O.gram_pinv(td.reshape(3, 4, 5, k))
    out = G.ref_rightmul(d, inv.numpy().astype(F32))[0]
    assert np.allclose(out, ddrg.reshape(k, p).t().numpy(), rtol=1e-4, atol=1e-6)


def test_pack_restatement():
    rng = np.random.default_rng(2)
    for b, k in ((33, 17), (70, 100), (64, 64)):
        v = rng.standard_normal((b, k)).astype(F32)
        for stream in ("f32", "bf16"):
            vp, vpt = G.ref_pack(v, b, k, stream)
            assert vp.shape == (C.round_up(b, 32), C.round_up(k, 16)) and vpt.shape == (G.code_rows(k), C.round_up(b, 32))
            assert np.array_equal(vp[:b, :k], v) and not vp[b:].any() and not vp[:, k:].any()
            want = torch.from_numpy(v).t()
            want = want.bfloat16().float() if stream == "bf16" else want
            assert np.array_equal(vpt[:k, :b], want.numpy()) and not vpt[k:].any() and not vpt[:, b:].any()
    assert [G.code_rows(k) for k in (1, 32, 33, 64, 65, 96, 97, 128)] == [32, 32, 64, 64, 128, 128, 128, 128]


def test_slab_sum_order():
    rng = np.random.default_rng(3)
    for n in (1, 2, 31, 32, 33, 70, 151):
        s = rng.standard_normal((n, 5)).astype(F32)
        acc = [np.zeros(5, F32) for _ in range(32)]
        for i in range(n):
            acc[i % 32] = acc[i % 32] + s[i]
        w = 16
        while w:
            for u in range(w):
                acc[u] = acc[u] + acc[u + w]
            w //= 2
        assert np.array_equal(G.slab_sum(s, n), acc[0])


# --------------------------------------------------------------------------------------------------------- the dispatch plan
def _L(kernel, targs, r0, rows, rows_p, t0, t1, tpw, nwg, grid, ks, slab, acc):
    return (kernel, targs, r0, rows, rows_p, t0, t1, tpw, nwg, grid, ks, slab, acc)


def _R(r0, rows, rows_p, nslabs):
    return ("reduce", r0, rows, rows_p, nslabs)


FM, FF, GD, GVM, GVF = "grad_fused_mfma", "grad_fused_f32", "grad_d_mfma", "grad_v_mfma", "grad_v_f32"
# (stream, B, P, K, want_d, want_v, aligned) -> (launches, nslabs, nchunks), worked out by hand from launch_grad for 256 CUs
PLAN_TABLE = {
    # launch_grad_fused_split: one 320-row chunk (RB = 2), three fast ranges and a slow one, halves of 49 / 48
    ("bf16", 300, 200, 97, True, True, True): ([
        _L(FM, ("bf16", 2, 8, 2, True, False, True), 0, 300, 320, 0, 3, 1, 3, 16, 49, 0, False),
        _L(FM, ("bf16", 2, 8, 2, False, False, True), 0, 300, 320, 3, 4, 1, 1, 16, 49, 3, False), _R(0, 300, 320, 4)], 4, 1),
    # launch_grad_fused_split, g unaligned: no fast range, the slow slabs start at 0
    ("bf16", 70, 72, 100, True, True, False): ([
        _L(FM, ("bf16", 2, 8, 1, False, False, True), 0, 70, 96, 0, 2, 1, 2, 16, 50, 0, False), _R(0, 70, 96, 2)], 2, 1),
    # launch_grad_fused<bf16, 2>: 512 rows (NW 8, RB 2), then 32 rows (NW 4) accumulating
    ("bf16", 544, 72, 33, True, True, True): ([
        _L(FM, ("bf16", 2, 8, 2, True, False, True), 0, 512, 512, 0, 1, 1, 1, 1, 0, 0, False),
        _L(FM, ("bf16", 2, 8, 2, False, False, True), 0, 512, 512, 1, 2, 1, 1, 1, 0, 1, False), _R(0, 512, 512, 2),
        _L(FM, ("bf16", 2, 4, 1, True, True, True), 512, 32, 32, 0, 1, 1, 1, 1, 0, 0, True),
        _L(FM, ("bf16", 2, 4, 1, False, True, True), 512, 32, 32, 1, 2, 1, 1, 1, 0, 1, True), _R(512, 32, 32, 2)], 0, 2),
    # launch_grad_fused<bf16, 2> with more tiles than workgroups: 300 fast tiles over 150 workgroups
    ("bf16", 33, 19208, 50, True, True, True): ([
        _L(FM, ("bf16", 2, 4, 1, True, False, True), 0, 33, 64, 0, 300, 2, 150, 150, 0, 0, False),
        _L(FM, ("bf16", 2, 4, 1, False, False, True), 0, 33, 64, 300, 301, 1, 1, 1, 0, 150, False), _R(0, 33, 64, 151)], 151, 1),
    # launch_grad_fused<f32, 1> generic (P % 32 != 0): 256 rows (NW 8), then 64 rows (NW 4) accumulating
    ("f32", 300, 200, 17, True, True, True): ([
        _L(FM, ("f32", 1, 8, 1, True, False, True), 0, 256, 256, 0, 3, 1, 3, 3, 0, 0, False),
        _L(FM, ("f32", 1, 8, 1, False, False, True), 0, 256, 256, 3, 4, 1, 1, 1, 0, 3, False), _R(0, 256, 256, 4),
        _L(FM, ("f32", 1, 4, 1, True, True, True), 256, 44, 64, 0, 3, 1, 3, 3, 0, 0, True),
        _L(FM, ("f32", 1, 4, 1, False, True, True), 256, 44, 64, 3, 4, 1, 1, 1, 0, 3, True), _R(256, 44, 64, 4)], 0, 2),
    # launch_grad_fused_f32<2, true>: four 256-row chunks
    ("f32", 1024, 96, 64, True, True, True): (list(itertools.chain.from_iterable(
        (_L(FF, (2, 8, r0 > 0, True), r0, 256, 256, 0, 3, 1, 3, 3, 0, 0, r0 > 0), _R(r0, 256, 256, 3)) for r0 in (0, 256, 512, 768))), 0, 4),
    # bf16, K > 64, Bp > 2048: launch_grad_d_lds (512-row chunks, the last of 1 row) + launch_grad_v<bf16, 4>
    ("bf16", 2049, 72, 100, True, True, True): (
        list(itertools.chain.from_iterable(
            (_L(FM, ("bf16", 4, 8, 2, True, r0 > 0, False), r0, 512, 512, 0, 1, 1, 1, 1, 0, -1, r0 > 0),
             _L(FM, ("bf16", 4, 8, 2, False, r0 > 0, False), r0, 512, 512, 1, 2, 1, 1, 1, 0, -1, r0 > 0)) for r0 in (0, 512, 1024, 1536)))
        + [_L(FM, ("bf16", 4, 8, 1, True, True, False), 2048, 1, 32, 0, 1, 1, 1, 1, 0, -1, True),
           _L(FM, ("bf16", 4, 8, 1, False, True, False), 2048, 1, 32, 1, 2, 1, 1, 1, 0, -1, True)]
        + list(itertools.chain.from_iterable(
            (_L(GVM, ("bf16", 4, 16, True), r0, 512, 512, 0, 1, 1, 1, 1, 0, 0, False),
             _L(GVM, ("bf16", 4, 16, False), r0, 512, 512, 1, 2, 1, 1, 1, 0, 1, False), _R(r0, 512, 512, 2)) for r0 in (0, 512, 1024, 1536)))
        + [_L(GVM, ("bf16", 4, 4, True), 2048, 1, 32, 0, 1, 1, 1, 1, 0, 0, False),
           _L(GVM, ("bf16", 4, 4, False), 2048, 1, 32, 1, 2, 1, 1, 1, 0, 1, False), _R(2048, 1, 32, 2)], 0, 5),
    # fp32, K > 64, P % 32 == 0: launch_grad_fused_f32<4, false> in 256-row chunks + the k-split grad_v_f32_kernel<2, .>
    ("f32", 600, 96, 128, True, True, True): ([
        _L(FF, (4, 8, False, False), 0, 256, 256, 0, 3, 1, 3, 3, 0, -1, False),
        _L(FF, (4, 8, True, False), 256, 256, 256, 0, 3, 1, 3, 3, 0, -1, True),
        _L(FF, (4, 8, True, False), 512, 88, 96, 0, 3, 1, 3, 3, 0, -1, True),
        _L(GVF, (2, 16), 0, 512, 512, 0, 3, 1, 3, 16, 64, 0, False), _R(0, 512, 512, 3),
        _L(GVF, (2, 4), 512, 88, 96, 0, 3, 1, 3, 16, 64, 0, False), _R(512, 88, 96, 3)], 0, 2),
    # fp32, K > 64, P % 32 != 0: launch_grad_d<f32, 4> + launch_grad_v<f32, 4> in 128-row chunks
    ("f32", 300, 72, 100, True, True, True): ([
        _L(GD, ("f32", 2, 4, True), 0, 300, 320, 0, 1, 1, 1, 1, 0, -1, False),
        _L(GD, ("f32", 2, 4, False), 0, 300, 320, 1, 2, 1, 1, 1, 0, -1, False)]
        + list(itertools.chain.from_iterable(
            (_L(GVM, ("f32", 4, 4, True), r0, rows, rp, 0, 1, 1, 1, 1, 0, 0, False),
             _L(GVM, ("f32", 4, 4, False), r0, rows, rp, 1, 2, 1, 1, 1, 0, 1, False), _R(r0, rows, rp, 2))
            for r0, rows, rp in ((0, 128, 128), (128, 128, 128), (256, 44, 64)))), 0, 3),
    # launch_grad_d<bf16, 1> alone: one fast 128-pixel tile and a tail
    ("bf16", 2049, 200, 10, True, False, True): ([
        _L(GD, ("bf16", 4, 1, True), 0, 2049, 2080, 0, 1, 1, 1, 1, 0, -1, False),
        _L(GD, ("bf16", 4, 1, False), 0, 2049, 2080, 1, 2, 1, 1, 1, 0, -1, False)], 0, 1),
    # launch_grad_v_f32<1> alone: rows_p = 96 -> 4 waves
    ("f32", 70, 96, 10, False, True, True): ([_L(GVF, (1, 4), 0, 70, 96, 0, 3, 1, 3, 3, 0, 0, False), _R(0, 70, 96, 3)], 3, 1),
    # launch_grad_d_lds alone, RB = 1
    ("bf16", 70, 72, 100, True, False, True): ([
        _L(FM, ("bf16", 4, 8, 1, True, False, False), 0, 70, 96, 0, 1, 1, 1, 1, 0, -1, False),
        _L(FM, ("bf16", 4, 8, 1, False, False, False), 0, 70, 96, 1, 2, 1, 1, 1, 0, -1, False)], 0, 1),
    # launch_grad_v<bf16, 4> alone: 16 + 4 waves in two chunks
    ("bf16", 600, 72, 113, False, True, True): ([
        _L(GVM, ("bf16", 4, 16, True), 0, 512, 512, 0, 1, 1, 1, 1, 0, 0, False),
        _L(GVM, ("bf16", 4, 16, False), 0, 512, 512, 1, 2, 1, 1, 1, 0, 1, False), _R(0, 512, 512, 2),
        _L(GVM, ("bf16", 4, 4, True), 512, 88, 96, 0, 1, 1, 1, 1, 0, 0, False),
        _L(GVM, ("bf16", 4, 4, False), 512, 88, 96, 1, 2, 1, 1, 1, 0, 1, False), _R(512, 88, 96, 2)], 0, 2),
}


@pytest.mark.parametrize("key", list(PLAN_TABLE), ids=lambda k: "-".join(str(x) for x in k))
def test_plan_against_the_table(key):
    stream, b, p, k, wd, wv, aligned = key
    want, nslabs, nchunks = PLAN_TABLE[key]
    plan = G.grad_plan(stream, b, p, k, wd, wv, aligned, NUM_CU)
    got = [("reduce", x.r0, x.rows, x.rows_p, x.nslabs) if isinstance(x, G.Reduce) else
           (x.kernel, x.targs, x.r0, x.rows, x.rows_p, x.t0, x.t1, x.tpw, x.nwg, x.grid, x.k_split, x.slab, x.acc) for x in plan.launches]
    assert got == want
    assert (plan.nslabs, plan.nchunks) == (nslabs, nchunks)


def test_pair_map_covers_every_half_once():
    for n in (1, 2, 7, 8, 9, 128):
        seen = [G.pair_map(bid) for bid in range(G.k_split_grid(n))]
        live = [x for x in seen if x[0] < n]
        assert sorted(live) == [(r, h) for r in range(n) for h in (0, 1)]
        for r, h in live:                                # the halves of a range sit 8 block ids apart
            assert seen.index((r, 1)) - seen.index((r, 0)) == 8


# every template instantiation launch_grad can launch, by hand from csrc/adil_contract.hip
_TF = (True, False)
INSTANTIATIONS = set(
    # launch_grad_d<T, AT>: PXT = 4 at AT = 1, else 2; bf16 at AT = 4 goes through LDS instead; FAST and the slow tail
    [(GD, (t, pxt, at, fast)) for t, pxt, at in (("bf16", 4, 1), ("bf16", 2, 2), ("f32", 4, 1), ("f32", 2, 2), ("f32", 2, 4)) for fast in _TF]
    # launch_grad_v<T, AT>: bf16 up to 16 waves; fp32 up to 8 waves at AT <= 2 and 4 waves at AT = 4
    + [(GVM, ("bf16", at, nw, fast)) for at in (1, 2, 4) for nw in (4, 8, 16) for fast in _TF]
    + [(GVM, ("f32", at, nw, fast)) for at, nw in ((1, 4), (1, 8), (2, 4), (2, 8), (4, 4)) for fast in _TF]
    # launch_grad_fused<T, AT> (AT <= 2; RB = 2 on bf16 only) and launch_grad_fused_split (bf16, AT = 2, NW = 8: among them)
    + [(FM, ("bf16", at, nw, rb, fast, acc, True)) for at in (1, 2) for nw, rb in ((4, 1), (8, 1), (8, 2)) for fast in _TF for acc in _TF]
    + [(FM, ("f32", at, nw, 1, fast, acc, True)) for at in (1, 2) for nw in (4, 8) for fast in _TF for acc in _TF]
    # launch_grad_d_lds
    + [(FM, ("bf16", 4, 8, rb, fast, acc, False)) for rb in (1, 2) for fast in _TF for acc in _TF]
    # launch_grad_fused_f32<AT, WV>
    + [(FF, (at, 8, acc, wv)) for at, wv in ((1, True), (2, True), (4, False)) for acc in _TF]
    # launch_grad_v_f32<AT>: AT = 4 runs the AT = 2 shape
    + [(GVF, (vat, nw)) for vat in (1, 2) for nw in (4, 8, 16)])


def _row_plans(r):
    r = G.resolve_row(r, NUM_CU)
    for w in r.wants:
        for acc in ((False, True) if "d" in w else (False,)):
            yield G.grad_plan(r.stream, r.b, r.p, r.k, "d" in w, "v" in w, r.off == 0, NUM_CU, acc)


def test_rows_reach_every_instantiation():
    assert len(INSTANTIATIONS) == 98
    reached = set()
    for r in G.ALL_ROWS:
        for plan in _row_plans(r):
            reached |= plan.instantiations()
    assert reached - INSTANTIATIONS == set(), "the plan launches something the hand-written list does not know"
    assert INSTANTIATIONS - reached == set(), sorted(INSTANTIATIONS - reached)


def test_rows_reach_two_tiles_per_workgroup():
    """Every kernel with a tile loop, in each of its forms: the generic fused kernel with and without grad_v, with and
    without the atom split; the fp32 fused kernel likewise; both grad_v kernels; Gram and D M^T."""
    seen = set()
    for r in G.ALL_ROWS:
        for plan in _row_plans(r):
            for x in plan.kernels():
                if x.tpw >= 2:
                    seen.add((x.kernel, x.outputs, x.k_split > 0))
    want = {(FM, "dv", False), (FM, "dv", True), (FM, "d", False), (FF, "dv", False), (FF, "d", False), (GVM, "v", False),
            (GVF, "v", False), (GVF, "v", True)}
    assert want <= seen, sorted(want - seen)
    assert G.gram_big_p(NUM_CU) == 9605 and G.gram_plan(9605, 50, NUM_CU)[1] == 2 and 9605 % 32 == 5
    assert G.gram_big_p(304) == 19205 and G.gram_plan(19205, 50, 304)[1] == 2
    assert G.rightmul_plan(G.rightmul_big_p(NUM_CU), 50, NUM_CU)[2] == 2


def test_rows_below_the_cap():
    for r in list(G.ALL_ROWS) + list(G.GAUSS_ROWS):
        r = G.resolve_row(r, NUM_CU)
        assert r.b * r.p * r.k <= CAP, G.row_id(r)
    assert len({G.row_id(r) for r in G.ALL_ROWS}) == len(G.ALL_ROWS)


# ------------------------------------------------------------------------------------ every GPU row through the emulation
def _params(rows):
    return [pytest.param(r, g, id=f"{G.row_id(r)}-{g}") for r in rows for g in G.GRIDS[r.stream]]


@pytest.mark.parametrize("r,grid", _params(G.ALL_ROWS))
def test_grad_rows_through_the_emulation(r, grid):
    G.check_grad_exact(G.resolve_row(r, NUM_CU), grid, run_grad(), NUM_CU)


@pytest.mark.parametrize("r", G.GAUSS_ROWS, ids=G.row_id)
def test_grad_gauss_through_the_emulation(r):
    worst = G.check_grad_gauss(G.resolve_row(r, NUM_CU), run_grad(), NUM_CU)
    print(f"\n{G.row_id(r)} gauss (emulation): worst err/bound = {worst:.4f}")
    assert 0 < worst < 1


@pytest.mark.parametrize("p", G.GRAM_P)
@pytest.mark.parametrize("grid", G.GRAM_GRIDS)
def test_gram_rows_through_the_emulation(p, grid):
    for k in G.GRAM_K:
        G.check_gram(p, k, grid, lambda d: G.emu_gram(d, NUM_CU))


@pytest.mark.parametrize("p", G.RIGHTMUL_P + (G.rightmul_big_p(NUM_CU),))
@pytest.mark.parametrize("grid", G.RIGHTMUL_GRIDS)
def test_rightmul_rows_through_the_emulation(p, grid):
    for k in (G.RIGHTMUL_K if p in G.RIGHTMUL_P else G.RIGHTMUL_BIG_K):
        G.check_rightmul(p, k, grid, lambda d, m: G.emu_rightmul(d, m, NUM_CU))


def test_gram_and_rightmul_gauss_through_the_emulation():
    for p, k in G.GRAM_GAUSS:
        w = G.check_gram_gauss(p, k, lambda d: G.emu_gram(d, NUM_CU))
        print(f"\ngram-P{p}-K{k} gauss (emulation): worst err/bound = {w:.4f}")
        assert 0 < w < 1
    for p, k in G.RIGHTMUL_GAUSS:
        w = G.check_rightmul_gauss(p, k, lambda d, m: G.emu_rightmul(d, m, NUM_CU))
        print(f"\nrightmul-P{p}-K{k} gauss (emulation): worst err/bound = {w:.4f}")
        assert 0 < w < 1


# ------------------------------------------------------------------------------------------------------------------ mutants
R33 = GradRow("f32", 70, 72, 33, ("dv", "d", "v"))
R33B = GradRow("bf16", 70, 72, 33, ("dv", "d", "v"))
R544 = GradRow("bf16", 544, 72, 33)
R300 = GradRow("bf16", 300, 200, 17)
R65 = GradRow("bf16", 70, 72, 65, ("dv", "d", "v"))
R1024 = GradRow("f32", 1024, 96, 64)
R600 = GradRow("f32", 600, 96, 128)
# mutant -> the leg (row, grid) that must fail
GRAD_MUTANTS = [
    ("drop_hh", R33, "narrow"), ("drop_hm", R33, "mid"), ("drop_mh", R33, "mid"), ("drop_mm", R33, "mid"),
    ("drop_lh", R33, "wide_g"), ("drop_hl", R33, "wide_v"), ("drop_hl", GradRow("f32", 70, 72, 33, ("v",)), "wide_d"),
    ("swap_ml", R33, "mid"), ("trunc_operand", R33B, "mid"), ("vpt_unconverted", R33B, "mid"),
    ("trunc_operand", GradRow("bf16", 70, 72, 33, ("v",)), "mid"),
    ("chunk_overwrites", R544, "narrow"), ("g_no_r0", R544, "narrow"), ("vpt_no_r0", R544, "narrow"),
    ("slow_slab_at_0", R300, "narrow"), ("slab_left_out", R300, "narrow"), ("slab_stride_rows", R300, "narrow"),
    ("half_starts_early", R65, "narrow"), ("half_unmasked", R65, "narrow"), ("pair_map", R65, "narrow"),
    ("pair_map", R600, "narrow"), ("half_starts_early", R600, "narrow"),
    ("pad_row_codes", R33, "narrow"), ("pix_tail_not_zeroed", R33, "narrow"), ("skip_last_group", R1024, "narrow"),
    ("skip_last_tile", R300, "narrow"), ("skip_last_tile", R1024, "narrow"),
]
assert all(r in G.ALL_ROWS or r._replace(wants=("dv", "d", "v")) in G.ALL_ROWS for _, r, _ in GRAD_MUTANTS)


@pytest.mark.parametrize("mutant,r,grid", GRAD_MUTANTS, ids=lambda x: x if isinstance(x, str) else G.row_id(x))
def test_grad_mutant_rejected(mutant, r, grid):
    G.check_grad_exact(r, grid, run_grad(), NUM_CU)
    with pytest.raises(AssertionError):
        G.check_grad_exact(r, grid, run_grad(mutant), NUM_CU)


# pinned as equivalent, with the reason
GRAD_EQUIVALENT = [
    ("trunc_operand", R33, "mid"),        # the three-way split of an fp32 stream: h + m + l is x under either rounding
    ("swap_ml", R33, "wide_g"),           # b = V, D one-hot: b.m = b.l = 0, the swap exchanges two zero planes
    ("swap_ml", R33, "wide_v"),           # a = g a power of two: a.m = a.l = 0, the set {a.h b.m, a.h b.l} is unchanged
    ("vpt_unconverted", R33B, "narrow"),  # seven-bit codes are bf16 numbers
]


@pytest.mark.parametrize("mutant,r,grid", GRAD_EQUIVALENT, ids=lambda x: x if isinstance(x, str) else G.row_id(x))
def test_grad_mutant_equivalent(mutant, r, grid):
    """An atom tail that is not zeroed is equivalent by construction in all three gradient kernels and in Gram: the
    columns >= kn of a workgroup's accumulators are never stored (emu_grad does not form them), so only D M^T, where
    the atoms are the reduction axis, has such a mutant."""
    G.check_grad_exact(r, grid, run_grad(mutant), NUM_CU)


GRAM_MUTANTS = [("drop_hh", 50, 17, "narrow"), ("drop_hm", 50, 17, "mid"), ("drop_mh", 50, 17, "mid"), ("drop_mm", 50, 17, "mid"),
                ("drop_lh", 432, 17, "wide"), ("drop_hl", 432, 17, "wide"), ("swap_ml", 50, 17, "mid"),
                ("pix_tail_not_zeroed", 50, 17, "narrow"), ("skip_last_tile", 9605, 17, "narrow"), ("slab_left_out", 432, 17, "narrow"),
                ("skip_last_group", 432, 17, "narrow"), ("upper_only", 50, 17, "narrow"), ("upper_only", 432, 65, "wide")]


@pytest.mark.parametrize("mutant,p,k,grid", GRAM_MUTANTS)
def test_gram_mutant_rejected(mutant, p, k, grid):
    G.check_gram(p, k, grid, lambda d: G.emu_gram(d, NUM_CU))
    with pytest.raises(AssertionError):
        G.check_gram(p, k, grid, lambda d: G.emu_gram(d, NUM_CU, mutant))


RIGHTMUL_MUTANTS = [("drop_hh", "narrow"), ("drop_hm", "mid"), ("drop_mh", "mid"), ("drop_mm", "mid"), ("drop_lh", "wide_d"),
                    ("drop_hl", "wide_m"), ("swap_ml", "mid"), ("m_not_transposed", "narrow"), ("atom_tail_not_zeroed", "narrow"),
                    ("skip_last_group", "narrow"), ("skip_last_tile", "narrow")]


@pytest.mark.parametrize("mutant,grid", RIGHTMUL_MUTANTS)
def test_rightmul_mutant_rejected(mutant, grid):
    p, k = 50, 32 if mutant == "skip_last_group" else 17
    G.check_rightmul(p, k, grid, lambda d, m: G.emu_rightmul(d, m, NUM_CU))
    with pytest.raises(AssertionError):
        G.check_rightmul(p, k, grid, lambda d, m: G.emu_rightmul(d, m, NUM_CU, mutant))


# ------------------------------------------------------------------------------------------------------------------- vacuity
def _plane_share(a, plane):
    a = np.asarray(a, F32)
    nz = a != 0
    return float((C.split3(a)[plane][nz] != 0).mean()) if nz.any() else 0.0


@pytest.mark.parametrize("r", [R33, R33B, GradRow("bf16", 2048, 72, 128), GradRow("f32", 33, 19208, 50)], ids=G.row_id)
def test_vacuity(r):
    """On the reference alone: the share of zero outputs, of operands that need the m and the l plane, and of bf16 ties."""
    for grid in G.GRIDS[r.stream]:
        o, gd0, gd1, gv = G.grad_reference(r, grid)
        zero_d, zero_v = float((gd0 == 0).mean()), float((gv == 0).mean())
        m = max(_plane_share(o.g, "m"), _plane_share(o.v, "m"), _plane_share(o.d, "m"))
        low = max(_plane_share(o.g, "l"), _plane_share(o.v, "l"), _plane_share(o.d, "l"))
        ties = float(np.mean([(C.sig_bits(a[a != 0]) == 9).mean() for a in (o.v, o.d)]))
        print(f"\n{G.row_id(r)}-{grid}: zero grad_d {zero_d:.3f} grad_v {zero_v:.3f}; operands needing m {m:.3f}, l {low:.3f}; "
              f"nine-bit V, D (bf16 ties) {ties:.3f}")
        # wide_v holds grad_d to the l plane and wide_d grad_v; the one-hot g leaves the other output sparse (not empty)
        assert zero_d < (1.0 if grid == "wide_d" else 0.7) and zero_v < (1.0 if grid == "wide_v" else 0.7), "mostly zeros"
        if grid == "narrow":
            assert m == 0 and low == 0 and zero_d < 0.05 and zero_v < 0.05
        if grid == "mid":
            assert ties > 0.15
            if r.stream == "f32":
                assert m > 0.5 and low == 0
        if grid.startswith("wide"):
            assert low > 0.9


def test_vacuity_gram_rightmul():
    for p, k in ((432, 50), (9605, 100)):
        for grid in G.GRAM_GRIDS:
            d, q, exact = G.gram_operands(p, k, grid)
            ref = G.ref_gram(d)[0]
            print(f"\ngram-P{p}-K{k}-{grid}: exact entries {exact.mean():.3f}, of them zero {(ref[exact] == 0).mean():.3f}; "
                  f"m {_plane_share(d, 'm'):.3f}, l {_plane_share(d, 'l'):.3f}")
            assert exact.mean() >= 0.74 and (ref[exact] != 0).any()
            assert (ref[exact] == 0).mean() < (0.05 if grid == "narrow" else 0.995)
    for grid in G.RIGHTMUL_GRIDS:
        d, m, q = G.rightmul_operands(432, 50, grid)
        ref = G.ref_rightmul(d, m)[0]
        print(f"\nrightmul-P432-K50-{grid}: zero outputs {(ref == 0).mean():.3f}")
        assert (ref == 0).mean() < 0.2
