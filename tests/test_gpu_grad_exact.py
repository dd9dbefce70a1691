"""adil_grad, adil_gram and adil_dict_rightmul (the third family of csrc/adil_contract.hip) through
dl_attack_on_imagenet_amd.ops against the restatements of tests/grad_reference.py, on two legs:

exact     operands on a grid (narrow, mid, wide one-hot) on which every product and every partial sum is an fp32 number:
          the kernels' bits must EQUAL the float64 restatement;
gaussian  g ~ N(0,1), V ~ 0.02 N(0,1), D ~ U[-1, 1], M ~ N(0,1)/sqrt(K) against float64 within grad_reference.grad_bound;
          the worst err / bound of each row is printed and a second call must return the same bits.

Every row is a call of a check_* function of grad_reference.py with a wrapper around ops as `run`;
tests/test_grad_reference_cpu.py calls the same functions with the numpy emulation, so each row is known to pass for a
correct kernel and to fail for the mutants listed there.  g, D, M, the codes and their packed forms sit in buffers that
are NaN everywhere else; grad_d is NaN-filled (or holds the on-grid initial contents) inside a sentinel buffer.  The
dispatch plan is taken for the device's CU count.  profiles/grad_exact.md lists the rows, the route each reaches and
what an MI355X made of them."""
import numpy as np
import pytest
import torch

import grad_reference as G
from test_gpu_contract_exact import dev, host, is_clean, nan_placed, ops, sentinel_out, tdtype
from test_gpu_routes import Placed

pytestmark = pytest.mark.gpu
F32 = torch.float32


def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------------------------------- wrapper around ops
def run_grad(c, plan):
    """One GradCase: the plain call (codes transposed inside adil_grad), a second identical call, and the call with vpt=
    from pack_codes(transposed=) and a deferred grad_v, which pack_codes then sums."""
    o = ops()
    dt = tdtype(c.stream)
    b, p = c.g.shape
    k = c.d.shape[1]
    g = nan_placed(dev(c.g).to(dt), c.off)
    d = nan_placed(dev(c.d), 0)
    v = nan_placed(dev(c.v), 0)
    vp0, vpt0 = o.pack_codes(v, None, b, transposed=dt)
    assert torch.equal(o.pack_codes(v, None, b), vp0), f"{c.name}: vp differs with transposed="
    vp, vpt = nan_placed(vp0, 0), nan_placed(vpt0, 0)
    outs = []

    def call(**kw):
        gd = None
        if c.want_d:
            gd = Placed(dev(c.init), 0) if c.init is not None else sentinel_out((p, k), F32, 0)
            outs.append(gd)
        rd, rv = o.grad(g, d, vp if c.want_d else None, b, want_d=c.want_d, want_v=c.want_v, grad_d=None if gd is None else gd.t,
                        accumulate_d=c.init is not None, **kw)
        assert (rd is None) == (not c.want_d) and (rd is None or rd.data_ptr() == gd.t.data_ptr())
        return (None if gd is None else host(gd.t)), rv

    res = dict(vp=host(vp0), vpt=host(vpt0))
    gd, gv = call()
    again_d, again_v = call()
    res["again"] = {}
    if c.want_d:
        res["grad_d"], res["again"]["grad_d"] = gd, again_d
    if c.want_v:
        assert gv.shape == (b, k)
        res["grad_v"], res["again"]["grad_v"] = host(gv), host(again_v)
    gd, gv = call(vpt=vpt if c.want_d else None, defer_v=c.want_v)
    if c.want_d:
        res["grad_d_vpt"] = gd
    if c.want_v:
        slab = isinstance(gv, o.SlabGrad)
        assert tuple(gv.shape) == (b, k)
        nslabs = gv.nslabs if slab else 0
        summed = o.pack_codes(gv, None, b) if slab else None
        if slab:
            assert not bool(summed[b:].any()) and not bool(summed[:, k:].any()), f"{c.name}: padding of the summed codes"
        res["deferred"] = dict(is_slab=slab, nslabs=nslabs, grad_v=host(summed[:b, :k]) if slab else host(gv))
    res["clean"] = all(is_clean(x) for x in outs)
    return res


def run_gram(d):
    return host(ops().gram(nan_placed(dev(d), 0)))


def run_rightmul(noncontiguous=False):
    def run(d, m):
        mt = dev(np.ascontiguousarray(m.T)).t() if noncontiguous else nan_placed(dev(m), 0)
        assert mt.is_contiguous() != (noncontiguous and m.shape[0] > 1)
        dd = nan_placed(dev(d), 0)
        out = ops().dict_rightmul(dd, mt)
        assert out.shape == dd.shape
        return host(out)
    return run


# ------------------------------------------------------------------------------------------------------------------ adil_grad
def _params(rows):
    return [pytest.param(r, g, id=f"{G.row_id(r)}-{g}") for r in rows for g in G.GRIDS[r.stream]]


@pytest.mark.parametrize("r,grid", _params(G.ALL_ROWS))
def test_grad_exact(r, grid):
    """Both outputs or the one the row names, without and with accumulation into an on-grid grad_d; vpt= and the deferred
    grad_v to the same bits; vp and vpt themselves: bits."""
    cu = num_cu()
    r = G.resolve_row(r, cu)
    if r.big_p:
        wd, wv = "d" in r.wants[0], "v" in r.wants[0]
        loops = [x for x in G.grad_plan(r.stream, r.b, r.p, r.k, wd, wv, True, cu).kernels() if x.kernel != "grad_d_mfma" and x.fast]
        assert loops and all(x.tpw >= 2 for x in loops), "the row does not walk two tiles per workgroup on this device"
    G.check_grad_exact(r, grid, run_grad, cu)


@pytest.mark.parametrize("r", G.GAUSS_ROWS, ids=G.row_id)
def test_grad_gauss(r):
    cu = num_cu()
    worst = G.check_grad_gauss(G.resolve_row(r, cu), run_grad, cu)
    print(f"\n{G.row_id(r)} gauss: worst err/bound = {worst:.4f}")


# ------------------------------------------------------------------------------------------------------------------ adil_gram
@pytest.mark.parametrize("grid", G.GRAM_GRIDS)
@pytest.mark.parametrize("p", G.GRAM_P)
def test_gram_exact(p, grid):
    """D^T D at every K of GRAM_K: bits, bit-symmetric; wide x wide entries within the derived bound."""
    if p == G.GRAM_P[-1]:
        p = G.gram_big_p(num_cu())
        assert G.gram_plan(p, 50, num_cu())[1] >= 2 and p % 32 == 5
    for k in G.GRAM_K:
        G.check_gram(p, k, grid, run_gram)


# ---------------------------------------------------------------------------------------------------------- adil_dict_rightmul
@pytest.mark.parametrize("grid", G.RIGHTMUL_GRIDS)
@pytest.mark.parametrize("p", G.RIGHTMUL_P + ("two-blocks",))
def test_rightmul_exact(p, grid):
    """D M^T at every K of RIGHTMUL_K (127 and 128 need more than 64 KB of dynamic LDS): bits.  The last P is above
    32 * 4 * (CU count): a workgroup walks two blocks.  M is non-contiguous (.t() of a matrix) on the narrow grid at P = 50."""
    ks = G.RIGHTMUL_K
    if p == "two-blocks":
        p, ks = G.rightmul_big_p(num_cu()), G.RIGHTMUL_BIG_K
        assert G.rightmul_plan(p, 50, num_cu())[2] == 2
    for k in ks:
        G.check_rightmul(p, k, grid, run_rightmul(noncontiguous=(grid == "narrow" and p == 50)))


def test_gram_rightmul_gauss():
    for p, k in G.GRAM_GAUSS:
        print(f"\ngram-P{p}-K{k} gauss: worst err/bound = {G.check_gram_gauss(p, k, run_gram):.4f}")
    for p, k in G.RIGHTMUL_GAUSS:
        print(f"\nrightmul-P{p}-K{k} gauss: worst err/bound = {G.check_rightmul_gauss(p, k, run_rightmul()):.4f}")
