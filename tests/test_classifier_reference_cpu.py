"""The comparators of tests/classifier_reference.py would notice a subtly wrong kernel: shown without a GPU.

For each kernel family of tests/test_gpu_classifier_routes.py the kernel is emulated on the CPU (fp32 accumulation in 16-
and 64-wide chunks of the reduction, in tap order, on the very operands the GPU table uses); the emulation passes both
legs, and every mutant of it is rejected by the exact leg.  Which mutants the gaussian leg rejects is printed, not
asserted.  Vacuity checks on the reference: every row has >= 25 % nonzero outputs, and every family has an exact-leg row
where >= 10 % of the outputs needed rounding and >= 1 % are exact ties."""
import pytest
import torch

import classifier_reference as R
import test_gpu_classifier_routes as T

CPU_BUDGET = 3e8          # multiply-adds of a row the emulation is run on (the reference alone runs on every row)


def _cost(r):
    c = r.cfg
    if r.family in ("pw_fwd", "pw_bwd"):
        return c["M"] * c["K"] * c["N"]
    if r.family in ("join_fwd", "join_bwd"):
        return 8 * c["M"] * c["W"] * c["W"]
    if r.family in ("conv3x3", "conv3x3_bwd", "s2_bwd"):
        return 9 * c["B"] * c["H"] * c["W"] * c["C"] * c["N"] // (4 if r.family == "s2_bwd" else 1)
    if r.family == "s2_fwd":
        return 9 * c["B"] * c["H"] * c["W"] * c["C"] * c["N"] // 4
    return 1


HAND = [r for r in T.ROUTES if not r.branch.startswith("product launch")]
SMALL = [r for r in HAND if _cost(r) <= CPU_BUDGET]
FAMILIES = sorted({r.family for r in T.ROUTES})
_ids = lambda rows: [r.name[:80] for r in rows]


def _emulate(r, o, chunk, mut=()):
    ar = R.Arith(R.F32, chunk, mut)
    return {k: R.finish(ar, v) for k, v in R.evaluate(r, ar, o).items() if not k.startswith("_")}


def _reference(r, o):
    return R.evaluate(r, R.Arith(), o)


def test_every_family_has_small_rows():
    assert {r.family for r in SMALL} == set(FAMILIES)


@pytest.mark.parametrize("r", SMALL, ids=_ids(SMALL))
def test_emulation_passes_both_legs(r):
    for leg in ("exact", "gaussian"):
        o = R.operands(r, leg)
        ref = _reference(r, o)
        for chunk in (16, 64):
            emu = _emulate(r, o, chunk)
            for k, got in emu.items():
                if leg == "exact":
                    R.compare_exact(f"{r.name} {k} chunk {chunk}", got, ref[k], R.geometry(r))
                else:
                    q = R.gaussian_ratio(got, ref[k])
                    assert q <= 1.0, (r.name, k, chunk, q)


def _sharp(rounded_ties):
    """Sort key of a (rounded, ties) pair: rows that meet both thresholds first, then the larger product."""
    rounded, ties = rounded_ties
    return (rounded >= 0.10 and ties >= 0.01, rounded * ties)


def test_vacuity_of_the_exact_leg():
    """On the reference alone, every row of the table: the premise, >= 25 % nonzero outputs; per family one row with
    >= 10 % really rounded outputs and >= 1 % exact ties."""
    best = {f: (0.0, 0.0) for f in FAMILIES}
    for r in T.ROUTES:
        ref = _reference(r, R.operands(r, "exact"))
        for k, o in ref.items():
            R.assert_premise(f"{r.name} {k}", o)
            if k.startswith("_"):
                continue
            nz, rounded, ties = R.stats(o)
            assert nz >= 0.25, (r.name, k, nz)
            best[r.family] = max(best[r.family], (rounded, ties), key=_sharp)
    print({f: (round(a, 3), round(b, 3)) for f, (a, b) in best.items()})
    for f, (rounded, ties) in best.items():
        assert rounded >= 0.10 and ties >= 0.01, (f, rounded, ties)


# --------------------------------------------------------------------------------------------------------------- mutants
def _differ(t):
    """First index whose value differs from its successor's."""
    return int((t[:-1] != t[1:]).nonzero()[0])


def _drop_k(r, o, channel=5):
    """Zero one weight of one output channel: its first nonzero one (of the centre tap for a 3x3 / 7x7 weight)."""
    key = {"pw_fwd": "w", "pw_bwd": "wt", "join_fwd": "w3", "join_bwd": "wt3"}.get(r.family, "w")
    t = o[key]
    if t.dim() == 4:                                                   # [N][C][k][k]: the output channel is N forward, C backward
        mid = t.shape[-1] // 2
        t = t[:, :, mid, mid] if r.family in ("conv3x3", "s2_fwd", "stem_fwd") else t[:, :, mid, mid].t()
    row = t[channel % t.shape[0]]
    row[int((row != 0).nonzero()[0])] = 0


def _neighbour(key):
    def apply(r, o):
        k = {"join_fwd": key + "3", "join_bwd": key + "3"}.get(r.family, key)
        i = _differ(o[k])
        o[k][i] = o[k][i + 1]
    return apply


def _res_last_row(r, o):
    o["res"][o["res"].shape[0] - 1] = 0


def _swap_tiles(out):
    for k, v in out.items():
        flat = v.reshape(-1, v.shape[-1]).clone()
        flat[:128], flat[128:256] = v.reshape(-1, v.shape[-1])[128:256], v.reshape(-1, v.shape[-1])[:128]
        out[k] = flat.reshape(v.shape)


def _gres_unwritten(out):
    """write_res taken from the wrong workgroups: the rows of the LAST 128-row tile of gres keep the canary."""
    g = out["gres"].clone()
    g[(g.shape[0] - 1) // 128 * 128:] = R.CANARY
    out["gres"] = g


CONVS = ("conv3x3", "conv3x3_bwd", "s2_fwd", "s2_bwd")
GEMMS = ("pw_fwd", "pw_bwd", "join_fwd", "join_bwd") + CONVS
# name: (families, row filter, operand edit, Arith switches, output edit)
MUTANTS = {
    "one k-term dropped for one output channel": (GEMMS + ("stem_fwd", "stem_bwd"), None, _drop_k, (), None),
    "one channel's scale taken from its neighbour": (("pw_fwd", "pw_bwd", "join_fwd", "join_bwd", "stem_fwd", "act_fwd", "act_bwd"),
                                                     None, _neighbour("scale"), (), None),
    "one channel's shift taken from its neighbour": (("pw_fwd", "join_fwd", "stem_fwd", "act_fwd"), lambda c: not c.get("zeros"),
                                                     _neighbour("shift"), (), None),
    "residual dropped for the last valid row of a tile": (("pw_fwd", "join_fwd"), lambda c: c.get("res") or "W" in c and "H" not in c, _res_last_row, (), None),
    "tap at w = 0 reads the previous row's last pixel": (("conv3x3", "conv3x3_bwd", "s2_fwd"), lambda c: c["H"] > 1 and c["W"] > 1, None,
                                                         ("no_wmask",), None),
    "tap at h = 0 reads the previous image": (("conv3x3", "conv3x3_bwd", "s2_bwd"), lambda c: c["B"] > 1, None, ("no_hmask",), None),
    "truncation instead of RNE": (GEMMS + ("stem_fwd", "stem_bwd", "act_fwd"), lambda c: c.get("dtype") != R.F32, None, ("trunc",), None),
    ">= 0 instead of > 0 in a mask": (("pw_bwd", "join_bwd", "act_bwd"), lambda c: c.get("relu", 1), None, ("ge_mask",), None),
    "g3 added at an odd pixel": (("pw_bwd",), lambda c: c.get("g3"), None, ("g3_odd",), None),
    "two 128-row tiles swapped": (("pw_fwd", "pw_bwd", "join_fwd", "join_bwd", "conv3x3", "s2_fwd"),
                                  lambda c: c.get("M", c.get("B", 0) * c.get("H", 0) * c.get("W", 0) // 4) >= 256, None, (), _swap_tiles),
    "gres of one row tile never written (write_res from the wrong ot)": (("pw_bwd",), lambda c: c.get("gres"), None, (), _gres_unwritten),
}
CASES = [(name, r) for name, (fams, flt, *_) in MUTANTS.items() for r in SMALL if r.family in fams and (flt is None or flt(r.cfg))]


def test_every_mutant_has_rows_in_every_family_it_applies_to():
    for name, (fams, *_rest) in MUTANTS.items():
        assert {r.family for n, r in CASES if n == name} == set(fams), name


def _clone(o):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in o.items()}


def _mutated(name, r, o):
    """The emulation's outputs under one mutant.  A dropped k-term of a dead channel (a ReLU prologue or an epilogue mask
    that is never positive there) changes nothing and is no mutant: the first channel from 5 on whose term matters."""
    _, _, edit, mut, post = MUTANTS[name]
    if edit is _drop_k:
        base = _emulate(r, o, 64)
        for channel in range(5, 13):
            om = _clone(o)
            _drop_k(r, om, channel)
            emu = _emulate(r, om, 64)
            if any(not torch.equal(emu[k], base[k]) for k in emu):
                return emu
        raise AssertionError(f"no live channel among 5..12 of {r.name}")
    om = _clone(o)
    if edit is not None:
        edit(r, om)
    emu = _emulate(r, om, 64, mut)
    if post is not None:
        post(emu)
    return emu


def _exact_rejects(r, emu, ref):
    def one(k):
        try:
            R.compare_exact(f"{r.name} {k}", emu[k], ref[k], R.geometry(r))
        except AssertionError:
            return True
        return False
    return any([one(k) for k in emu])


@pytest.mark.parametrize("name,r", CASES, ids=[f"{n[:28]}-{r.name[:50]}" for n, r in CASES])
def test_exact_leg_rejects_mutant(name, r):
    o = R.operands(r, "exact")
    exact = _exact_rejects(r, _mutated(name, r, o), _reference(r, o))
    o = R.operands(r, "gaussian")
    ref = _reference(r, o)
    gaussian = max(R.gaussian_ratio(got, ref[k]) for k, got in _mutated(name, r, o).items()) > 1.0
    print(f"{name} on {r.name}: exact leg rejects: {exact}, gaussian leg rejects: {gaussian}")
    assert exact, f"the exact leg accepted the mutant `{name}` on {r.name}"


# ------------------------------------------------------------------------------- the restatements against torch's own ops
def _close(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert float((a - b).abs().max()) <= 1e-9 * max(1.0, float(b.abs().max())), what


def test_convolution_restatements_agree_with_torch():
    """The fp64 restatements of the 3x3 / 7x7 convolutions and of their input gradients against torch.nn.functional
    convolutions and autograd in float64 (NCHW), on gaussian operands."""
    import torch.nn.functional as F
    ar = R.Arith()
    g = R.Gen("cross-check", "gaussian")
    nchw = lambda t: t.double().permute(0, 3, 1, 2)
    x, w = g.act(2, 6, 8, 64), g.weight(128, 64, 3, 3)
    for stride, fwd, bwd in ((1, R.conv3x3, lambda gy: R.conv3x3_bwd(ar, gy, w)),
                             (2, R.conv3x3_s2_fwd, lambda gy: R.conv3x3_s2_bwd(ar, gy, w, 6, 8))):
        xr = nchw(x).clone().requires_grad_(True)
        y = F.conv2d(xr, w.double(), stride=stride, padding=1)
        _close(nchw(fwd(ar, x, w)["y"].pre), y.detach(), f"3x3 stride {stride} forward")
        gy = g.act(*y.permute(0, 2, 3, 1).shape)
        (gx,) = torch.autograd.grad(y, xr, nchw(gy))
        _close(nchw(bwd(gy)["gx"].pre), gx, f"3x3 stride {stride} input gradient")
    # the packings the kernels take: conv3x3 on the flipped packing IS the input gradient
    wf = R.pack_taps_flipped(w).reshape(64, 3, 3, 128).permute(0, 3, 1, 2)
    gy = g.act(2, 6, 8, 128)
    _close(R.conv3x3(ar, gy, wf)["y"].pre, R.conv3x3_bwd(ar, gy, w)["gx"].pre, "flipped packing")
    # stem: fp32 image, mean / inv_std, 7x7 stride 2
    o = R.operands(R.Route("stem_fwd", "", dict(B=2, H=20, W=36, dtype=R.F32)), "gaussian")
    mean = torch.tensor(o["mean"]).view(1, 3, 1, 1)
    istd = torch.tensor(o["inv_std"]).view(1, 3, 1, 1)
    xn = ((o["x"] - mean) * istd).bfloat16().double().requires_grad_(True)
    y = F.conv2d(xn, o["w"].double(), stride=2, padding=3)
    ref = R.stem_fwd(ar, **o)["y"]
    _close(nchw(ref.pre), (y * o["scale"].double().view(1, 64, 1, 1) + o["shift"].double().view(1, 64, 1, 1)).detach(), "stem forward")
    gy = g.act(2, 10, 18, 64)
    (gx,) = torch.autograd.grad(y, xn, nchw(gy))
    _close(R.stem_bwd(ar, gy, o["w"], o["inv_std"], 20, 36, R.F32)["gx"].pre, gx * istd.double(), "stem input gradient")


def test_pointwise_and_join_restatements_agree_with_autograd():
    """pw_fwd / pw_bwd against autograd of the same formula in float64 (no bf16 rounding: relu masks from the forward),
    the stride-2 gather and g3 against slicing, and the join restated directly against two pointwise restatements."""
    ar = R.Arith()
    g = R.Gen("cross-check-pw", "gaussian")
    B, OH, OW, K, N = 2, 3, 5, 64, 128
    x4 = g.act(B, 2 * OH, 2 * OW, K)
    w, scale, shift = g.weight(N, K), g.scale(N), g.shift(N)
    sub = R.pw_fwd(ar, x4.reshape(-1, K), w, scale, shift, relu=0, sub_w=OW, sub_hw=OH * OW, M=B * OH * OW)["y"].pre
    _close(sub, R.pw_fwd(ar, x4[:, ::2, ::2].reshape(-1, K), w, scale, shift, relu=0)["y"].pre, "stride-2 gather")
    M = B * 4 * OH * OW
    xin, ps, pb, res = g.act(M, K), g.scale(K), g.shift(K), g.act(M, N)
    xr, rr = xin.double().requires_grad_(True), res.double().requires_grad_(True)
    xp = torch.relu(xr * ps.double() + pb.double())
    y = torch.relu(xp @ w.double().t() * scale.double() + shift.double() + rr)
    gy, g2, g3 = g.act(M, N), g.act(M, N), g.act(M // 4, N)
    up = torch.zeros(B, 2 * OH, 2 * OW, N, dtype=torch.float64)
    up[:, ::2, ::2] = g3.double().reshape(B, OH, OW, N)
    gx, gres = torch.autograd.grad(y, (xr, rr), gy.double() + g2.double() + up.reshape(M, N))
    out = R.pw_bwd(ar, gy, w.t().contiguous(), scale, y=y.detach(), g2=g2, relu=1, xin=xin, pscale=ps, pshift=pb, g3=g3, sub_w=OW,
                   sub_hw=OH * OW)
    assert float((R.finish(ar, out["gres"]) - gres).abs().max()) <= 2.0 ** -7 * float(gres.abs().max())
    # gx: the restatement rounds gz and gx to bf16 on the way; autograd does not
    err = (torch.where(out["gx"].mask, out["gx"].pre, torch.zeros(())) - gx).abs()
    assert float(err.max()) <= 2.0 ** -6 * float(gx.abs().max()), float(err.max())
    # join = conv3 (prologue, residual, ReLU) then conv1 (ReLU), forward and backward
    r = R.Route("join_fwd", "", dict(M=200, W=64))
    for leg in ("exact", "gaussian"):
        o = R.operands(r, leg)
        j = R.join_fwd(ar, **o)
        a = R.pw_fwd(ar, o["h2raw"], o["w3"], o["scale3"], o["shift3"], o["res"], 1, o["pscale2"], o["pshift2"])["y"]
        out = R.finish(ar, a)
        b = R.pw_fwd(ar, out.bfloat16(), o["w1"], o["scale1"], o["shift1"], None, 1)["y"]
        assert torch.equal(R.finish(ar, j["out"]), out) and torch.equal(R.finish(ar, j["h1"]), R.finish(ar, b)), leg
        ob = R.operands(R.Route("join_bwd", "", dict(M=200, W=64)), leg)
        jb = R.join_bwd(ar, **ob)
        t = R.finish(ar, R.pw_bwd(ar, ob["g_h1"], ob["wt1"], ob["scale1"], y=ob["h1"], relu=1, want_gres=False)["gx"])
        two = R.pw_bwd(ar, t.bfloat16(), ob["wt3"], ob["scale3"], y=ob["out"], g2=ob["g_out"], relu=1, xin=ob["h2raw"],
                       pscale=ob["pscale2"], pshift=ob["pshift2"])
        for k in ("gres", "gx"):
            assert torch.equal(R.finish(ar, jb[k]), R.finish(ar, two[k])), (leg, k)
