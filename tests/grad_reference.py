"""Restatements, a dispatch plan, kernel emulations, operand generators and row checks for the third family of
csrc/adil_contract.hip: adil_grad (grad_d = g^T V, grad_v = g D), adil_gram (G = D^T D) and adil_dict_rightmul
(out = D M^T).  numpy / torch CPU only: no GPU, no library.  The layout is that of contract_reference.py, whose number
formats, emu_contract and grids are used here.

restatements   float64, on the operands the kernels multiply: bf16 streams g as given, rne_bf16(V) for grad_d and
               rne_bf16(D) for grad_v; fp32 streams exact.  ref_pack restates pack_codes(..., transposed=dtype).
grad_plan      launch_grad and its launchers in plain Python: the list of kernel launches of one adil_grad call, each
               with its template arguments, row chunk, tile range, workgroup spread, atom split, slab base and whether
               it accumulates; the slab count a deferred grad_v reports and the number of row chunks.
emulations     emu_grad follows the plan launch by launch and workgroup by workgroup into FLAT buffers (grad_d inside
               a sentinel buffer, the slab area full of NaN), so a wrong offset lands where the kernel's would; every
               contraction goes through emu_contract in k-groups of 16.  emu_gram, emu_rightmul likewise.  Each takes a
               `mutant` name and then computes the deliberately wrong variant the rows must reject.
checks         one per family, taking a `run` callable (ops on the GPU, the emulation on the CPU).

exact legs     every product and every partial sum is an fp32 number, so any summation order gives the same bits.  The
               premise is asserted on the reference alone, in float64: every term is a multiple of the output's quantum
               q and sum |terms| + |init| < 2^24 q.  Then the bits must be EQUAL (only the sign of a zero is not
               compared; no element is excluded).  Grids (reduction axis: B for grad_d, P for grad_v and Gram, K for
               D M^T):
                 narrow  g = i 2^-7 (|i| <= 127), V = j 2^-7 (|j| <= 7, fewer for long B), D = i 2^-7 (|i| <= 127, fewer
                         for long P: the range is halved until the premise holds), q = 2^-14; init = n 2^-14, |n| <= 4096.
                 mid     MID_CLASSES (a, c) by batch row and by pixel: g[b, p] = odd a-bit integers 2^-a where row and
                         pixel share a class (0 elsewhere), V[b, :] = odd c-bit integers 2^(a-23), D[p, :] likewise; every
                         column of V / D has at most MID_NNZ non-zeros along the reduction axis: q = 2^-23, hh, hm, mh,
                         mm all contribute, nine-bit V / D are bf16 ties (bf16 streams: g is rounded to bf16 when it
                         is made, the reference rounds V and D).
                 wide_g  g = odd 24-bit integers 2^-24 against one +-2^-2 per column of V and one +-2^-6 per column of
                         D: needs a.l b.h in both outputs.
                 wide_v  V = odd 24-bit integers 2^-29 against one +-2^-2 per pixel column of g: needs a.h b.l in grad_d;
                         D narrow, so grad_v is exact too.
                 wide_d  D = odd 24-bit integers 2^-24 against one +-2^-6 per row of g: needs a.h b.l in grad_v; V narrow.
gaussian leg   g ~ N(0,1), V ~ 0.02 N(0,1), D ~ U[-1,1], M ~ N(0,1)/sqrt(K) against float64 within grad_bound.
"""
from typing import NamedTuple, Optional

import numpy as np

import contract_reference as C
from contract_reference import F32, U24, SENTINEL, emu_contract, low_quantum, operands64, rne_bf16, round_up, seed_of, trunc_bf16
from update_reference import assert_bits_equal, assert_within

GV_TW = 64
MAX_ATOMS = 128


def grad_at(k):
    a = (k + 31) // 32
    return a if a <= 2 else 4


def code_rows(k):
    """adil_grad_code_rows."""
    return grad_at(k) * 32


# ============================================================================================================== restatements
def ref_pack(v, b, k, stream, mutant=None):
    """pack_codes(v, None, b, transposed=dtype): vp [round_up(B, 32)][round_up(K, 16)] fp32 and vpt [code_rows(K)]
    [round_up(B, 32)] = vp^T converted to the stream type (returned as float32 values); all padding zero.
    mutants: vpt_unconverted (bf16 streams: vpt keeps the fp32 codes) | trunc_operand (converted by truncation)."""
    bp, kp = round_up(b, 32), round_up(k, 16)
    vp = np.zeros((bp, kp), F32)
    vp[:b, :k] = np.asarray(v, F32)[:b, :k]
    vpt = np.zeros((code_rows(k), bp), F32)
    vpt[:kp] = vp.T
    if stream == "bf16" and mutant != "vpt_unconverted":
        vpt = trunc_bf16(vpt) if mutant == "trunc_operand" else rne_bf16(vpt)
    return vp, vpt


def ref_grad(g, d, v, stream, init=None):
    """(grad_d (P, K), S_d, grad_v (B, K), S_v) in float64; S = sum |terms| (+ |init|)."""
    g64 = np.asarray(g, F32).astype(np.float64)
    v64, d64 = operands64(v, stream), operands64(d, stream)
    gd, sd = g64.T @ v64, np.abs(g64).T @ np.abs(v64)
    if init is not None:
        gd, sd = gd + init.astype(np.float64), sd + np.abs(init.astype(np.float64))
    return gd, sd, g64 @ d64, np.abs(g64) @ np.abs(d64)


def ref_gram(d):
    d64 = np.asarray(d, F32).astype(np.float64)
    return d64.T @ d64, np.abs(d64).T @ np.abs(d64)


def ref_rightmul(d, m):
    d64, m64 = np.asarray(d, F32).astype(np.float64), np.asarray(m, F32).astype(np.float64)
    return d64 @ m64.T, np.abs(d64) @ np.abs(m64).T


# ============================================================================================================ the dispatch plan
class Launch(NamedTuple):
    """One kernel launch of adil_grad.  kernel + targs: the instantiation, template arguments in the order of the source
    (stream types as "bf16" / "f32").  Rows [r0, r0 + rows_p) of the padded batch, `rows` of them real.  Pixel tiles of
    `tw` pixels [t0, t1), fast: the vector-load variant; nwg workgroups (tile ranges) of tpw tiles each, `grid` blocks
    launched (k_split > 0: two per range, in the 16-per-8 map).  slab: first slab of this launch (in slabs of
    rows_p x K floats), -1: writes none.  acc: adds to grad_d.  outputs: "d", "v" or "dv"."""
    kernel: str
    targs: tuple
    r0: int
    rows: int
    rows_p: int
    tw: int
    t0: int
    t1: int
    fast: bool
    tpw: int
    nwg: int
    grid: int
    k_split: int
    slab: int
    acc: bool
    outputs: str


class Reduce(NamedTuple):
    """grad_v_reduce_kernel behind one row chunk: nslabs slabs of rows_p x K into rows [r0, r0 + rows) of grad_vb."""
    r0: int
    rows: int
    rows_p: int
    nslabs: int


class Plan(NamedTuple):
    launches: tuple       # Launch and Reduce entries in launch order
    nslabs: int           # what a deferred grad_v reports: > 0 exactly when ONE row chunk makes the slabs
    nchunks: int          # row chunks of the pass that makes grad_v (of the grad_d pass when grad_v is not wanted)

    def kernels(self):
        return [x for x in self.launches if isinstance(x, Launch)]

    def instantiations(self):
        return {(x.kernel, x.targs) for x in self.kernels()}


def _tile_split(p, tw, vec):
    ntiles = (p + tw - 1) // tw
    return ntiles, (p // tw if vec else 0)


def _spread(n, slots):
    tpw = (n + slots - 1) // slots if n > 0 else 1
    return tpw, ((n + tpw - 1) // tpw if n > 0 else 0)


def k_split_grid(nranges):
    return 16 * ((nranges + 7) // 8)


def pair_map(bid, mutant=None):
    """Block id -> (tile range, atom half) of a k-split launch: the halves of a range sit 8 block ids apart."""
    if mutant == "pair_map":
        return (bid >> 4) * 8 + (bid & 15), (bid >> 3) & 1
    return (bid >> 4) * 8 + (bid & 7), (bid >> 3) & 1


def grad_plan(stream, b, p, k, want_d=True, want_v=True, aligned=True, num_cu=256, accumulate=False):
    """launch_grad<T, AT> of csrc/adil_contract.hip restated (see Launch, Reduce, Plan)."""
    assert stream in ("bf16", "f32") and 0 < k <= MAX_ATOMS and (want_d or want_v)
    at, bp = grad_at(k), round_up(b, 32)
    bf = stream == "bf16"
    half_cu = max(num_cu // 2, 1)
    vec = lambda m: p % m == 0 and aligned
    out = []
    state = dict(nslabs=0, chunks_d=0, chunks_v=0)

    def row_chunks(chunk, nslabs, run, makes):
        n = 0
        for r0 in range(0, bp, chunk):
            rows_p = min(bp - r0, chunk)
            rows = min(b - r0, rows_p)
            run(r0, rows, rows_p, bool(accumulate) or r0 > 0)
            if nslabs > 0:
                if bp <= chunk:
                    state["nslabs"] = nslabs
                out.append(Reduce(r0, rows, rows_p, nslabs))
            n += 1
        for key in makes:
            state[key] = n

    def fused_chunk(t, at_, nw, rb, wv, r0, rows, rows_p, acc, ts, f, s, ks=0):
        ntiles, nfast = ts
        for fast, t0, t1, (tpw, nwg), slab in ((True, 0, nfast, f, 0), (False, nfast, ntiles, s, f[1])):
            if nwg > 0:
                out.append(Launch("grad_fused_mfma", (t, at_, nw, rb, fast, acc, wv), r0, rows, rows_p, GV_TW, t0, t1, fast, tpw,
                                  nwg, k_split_grid(nwg) if ks else nwg, ks, slab if wv else -1, acc, "dv" if wv else "d"))

    def fused_split():
        ts = _tile_split(p, GV_TW, vec(8))
        f, s = _spread(ts[1], half_cu), _spread(ts[0] - ts[1], half_cu)
        kh = (k + 1) // 2
        row_chunks(512, f[1] + s[1], lambda r0, rows, rows_p, acc: fused_chunk(
            stream, 2, 8, 2 if rows_p > 256 else 1, True, r0, rows, rows_p, acc, ts, f, s, kh), ("chunks_d", "chunks_v"))

    def fused():
        ts = _tile_split(p, GV_TW, vec(8))
        f, s = _spread(ts[1], num_cu), _spread(ts[0] - ts[1], num_cu)
        max_rows = 512 if bf else 256

        def run(r0, rows, rows_p, acc):
            nblk = rows_p // 32
            nw, rb = (8, 2) if (bf and nblk > 8) else ((8, 1) if nblk > 4 else (4, 1))
            fused_chunk(stream, at, nw, rb, True, r0, rows, rows_p, acc, ts, f, s)
        row_chunks(max_rows, f[1] + s[1], run, ("chunks_d", "chunks_v"))

    def fused_f32(at_, wv):
        nt = p // 32
        tpw, nwg = _spread(nt, num_cu)
        row_chunks(256, nwg if wv else 0, lambda r0, rows, rows_p, acc: out.append(Launch(
            "grad_fused_f32", (at_, 8, acc, wv), r0, rows, rows_p, 32, 0, nt, True, tpw, nwg, nwg, 0, 0 if wv else -1, acc,
            "dv" if wv else "d")), ("chunks_d", "chunks_v") if wv else ("chunks_d",))

    def grad_d_lds():
        ts = _tile_split(p, GV_TW, vec(8))
        f, s = _spread(ts[1], num_cu), _spread(ts[0] - ts[1], num_cu)
        row_chunks(512, 0, lambda r0, rows, rows_p, acc: fused_chunk(
            stream, 4, 8, 2 if rows_p > 256 else 1, False, r0, rows, rows_p, acc, ts, f, s), ("chunks_d",))

    def grad_d():
        pxt = 4 if at == 1 else 2
        ntiles, nfast = _tile_split(p, pxt * 32, vec(4))
        for fast, t0, t1 in ((True, 0, nfast), (False, nfast, ntiles)):
            if t1 > t0:
                out.append(Launch("grad_d_mfma", (stream, pxt, at, fast), 0, b, bp, pxt * 32, t0, t1, fast, 1, t1 - t0,
                                  (t1 - t0 + 3) // 4, 0, -1, bool(accumulate), "d"))
        state["chunks_d"] = 1

    def grad_v_f32():
        vat = 2 if at == 4 else at
        nt = p // 32
        ks = (k + 1) // 2 if at == 4 else 0
        tpw, nwg = _spread(nt, half_cu if at == 4 else num_cu)
        row_chunks(512, nwg, lambda r0, rows, rows_p, acc: out.append(Launch(
            "grad_v_f32", (vat, 16 if rows_p > 256 else (8 if rows_p > 128 else 4)), r0, rows, rows_p, 32, 0, nt, True, tpw, nwg,
            k_split_grid(nwg) if ks else nwg, ks, 0, False, "v")), ("chunks_v",))

    def grad_v():
        kmax = 16 if bf else (8 if at <= 2 else 4)
        ts = _tile_split(p, GV_TW, vec(8))
        f, s = _spread(ts[1], num_cu), _spread(ts[0] - ts[1], num_cu)

        def run(r0, rows, rows_p, acc):
            nwaves = rows_p // 32
            nw = 16 if (kmax >= 16 and nwaves > 8) else (8 if (kmax >= 8 and nwaves > 4) else 4)
            for fast, t0, t1, (tpw, nwg), slab in ((True, 0, ts[1], f, 0), (False, ts[1], ts[0], s, f[1])):
                if nwg > 0:
                    out.append(Launch("grad_v_mfma", (stream, at, nw, fast), r0, rows, rows_p, GV_TW, t0, t1, fast, tpw, nwg, nwg,
                                      0, slab, False, "v"))
        row_chunks(kmax * 32, f[1] + s[1], run, ("chunks_v",))

    both = want_d and want_v
    done = False
    if at == 4 and bf and both and bp <= 4 * 512:
        fused_split()
        done = True
    elif at <= 2 and both and bp <= 4 * (512 if bf else 256):
        if not bf and vec(32):
            fused_f32(at, True)
        else:
            fused()
        done = True
    if not done:
        if want_d:
            if at == 4 and bf:
                grad_d_lds()
            elif at == 4 and vec(32):
                fused_f32(4, False)
            else:
                grad_d()
        if want_v:
            if not bf and vec(32):
                grad_v_f32()
            else:
                grad_v()
    return Plan(tuple(out), state["nslabs"] if want_v else 0, state["chunks_v"] if want_v else state["chunks_d"])


def gram_plan(p, k, num_cu=256):
    """(tiles of 32 pixels, tiles per workgroup, workgroups = slabs) of adil_gram."""
    nt = (p + 31) // 32
    tpw, nwg = _spread(nt, num_cu)
    return nt, tpw, nwg


def rightmul_plan(p, k, num_cu=256):
    """(32-pixel blocks, workgroups, blocks the first workgroup walks) of adil_dict_rightmul."""
    nblocks = (p + 31) // 32
    grid = min(nblocks, 4 * num_cu)
    return nblocks, grid, (nblocks + grid - 1) // grid


# ================================================================================================================ emulations
CONTRACT_MUTANTS = C.DROP_MUTANTS + ("swap_ml", "trunc_operand", "skip_last_group")


def slab_sum(slabs, nslabs):
    """slab_sum of adil_common.h on an array whose first axis counts the slabs: slab s goes to accumulator s % 32 in
    order, the 32 accumulators meet in a pairwise tree; fp32 throughout."""
    acc = np.zeros((32,) + slabs.shape[1:], F32)
    with np.errstate(all="ignore"):
        for s in range(nslabs):
            acc[s % 32] = acc[s % 32] + slabs[s]
        w = 16
        while w >= 1:
            acc[:w] = acc[:w] + acc[w:2 * w]
            w //= 2
    return acc[0]


class GradCase(NamedTuple):
    """One adil_grad call.  g (B, P) float32 holding stream-exact values; d (P, K); v (B, K); init: grad_d's contents
    before an accumulating call (None: no accumulation); off: elements g sits past a 16-byte boundary."""
    name: str
    g: np.ndarray
    d: np.ndarray
    v: np.ndarray
    stream: str
    want_d: bool = True
    want_v: bool = True
    init: Optional[np.ndarray] = None
    off: int = 0


def case_plan(c, num_cu):
    b, p = c.g.shape
    return grad_plan(c.stream, b, p, c.d.shape[1], c.want_d, c.want_v, c.off == 0, num_cu, c.init is not None)


GD_PAD = 256         # sentinel elements before and behind grad_d in the emulation's flat buffer
AT_ARG = {"grad_fused_mfma": 1, "grad_v_mfma": 1, "grad_fused_f32": 0, "grad_v_f32": 0, "grad_d_mfma": 2}   # AT among targs


def emu_grad(c, num_cu=256, mutant=None):
    """adil_grad as the plan launches it.  grad_d lives in a flat sentinel buffer and the slabs in a flat NaN area of the
    workspace's size, addressed the way the kernels address them.  Returns the keys check_grad_exact reads.
    mutants (beside emu_contract's): chunk_overwrites | g_no_r0 | vpt_no_r0 | slow_slab_at_0 | slab_left_out |
    slab_stride_rows | half_starts_early | half_unmasked | pair_map | pad_row_codes | pix_tail_not_zeroed |
    skip_last_tile | vpt_unconverted."""
    b, p = c.g.shape
    k = c.d.shape[1]
    bp, ka = round_up(b, 32), code_rows(k)
    plan = case_plan(c, num_cu)
    cm = mutant if mutant in CONTRACT_MUTANTS else None
    g = np.asarray(c.g, F32)
    d = np.asarray(c.d, F32)
    vp, vpt = ref_pack(c.v, b, k, c.stream, mutant)
    if mutant == "pad_row_codes":                    # rows >= B are read from row B - 1: their codes must be zero
        vpt[:, b:] = vpt[:, b - 1:b]
    gdbuf = np.full(GD_PAD + p * k + GD_PAD, SENTINEL, F32)
    gdbuf[GD_PAD:GD_PAD + p * k] = np.nan if c.init is None else np.asarray(c.init, F32).reshape(-1)
    slab_rows = min(bp, 512)
    slab = np.full((2 * num_cu + 2) * slab_rows * ka + 4096, np.nan, F32)
    gv = np.full((b, k), np.nan, F32)
    vstream = "raw" if c.stream == "bf16" else "f32"      # grad_d: vpt is already converted, g is stream-exact
    vm = cm if cm != "trunc_operand" or c.stream == "f32" else None

    def rows_of(x, r0g, rows):                        # g + r0 P with B = rows: row index clamped to the last real one
        idx = np.minimum(np.arange(x.rows_p), rows - 1) + r0g
        return g[idx]

    with np.errstate(all="ignore"):
        for x in plan.launches:
            if isinstance(x, Reduce):
                ns = x.nslabs - (1 if mutant == "slab_left_out" else 0)
                sl = slab[:x.nslabs * x.rows_p * k].reshape(x.nslabs, x.rows_p, k)
                gv[x.r0:x.r0 + x.rows] = slab_sum(sl, ns)[:x.rows]
                continue
            r0g = 0 if (mutant == "g_no_r0") else x.r0
            r0v = 0 if (mutant == "vpt_no_r0") else x.r0
            gch = rows_of(x, r0g, x.rows)             # rows_p x P
            acc = x.acc and not (mutant == "chunk_overwrites" and x.r0 > 0)
            ka_l = x.targs[AT_ARG[x.kernel]] * 32     # atom columns this instantiation holds
            slab0 = 0 if (mutant == "slow_slab_at_0") else max(x.slab, 0)
            for bid in range(x.grid):
                rng_, k0, kn = bid, 0, k
                if x.k_split:
                    rng_, half = pair_map(bid, mutant)
                    if rng_ >= x.nwg:
                        continue
                    k0 = (x.k_split - (1 if mutant == "half_starts_early" else 0)) if half else 0
                    kn = k - x.k_split if half else x.k_split
                if x.kernel == "grad_d_mfma":         # a wave per tile, four per block
                    ta, tb = x.t0 + 4 * bid, min(x.t1, x.t0 + 4 * bid + 4)
                else:
                    ta = x.t0 + rng_ * x.tpw
                    tb = min(x.t1, ta + x.tpw)
                if mutant == "skip_last_tile" and tb == x.t1:
                    tb -= 1
                px = np.arange(ta * x.tw, max(tb, ta) * x.tw)
                pxc, valid = np.minimum(px, p - 1), px < p
                gblk = gch[:, pxc]                    # pixels beyond P: clamped loads
                ncol = min(ka_l, kn) if mutant != "half_unmasked" else min(ka_l, ka - k0)
                if "v" in x.outputs:                  # ---- the slab of this workgroup
                    cols = np.minimum(k0 + np.arange(ncol), k0 + kn - 1) if mutant != "half_unmasked" else np.minimum(k0 + np.arange(ncol), k - 1)
                    dt = d[pxc][:, cols]
                    if mutant != "pix_tail_not_zeroed":
                        dt = dt * valid[:, None].astype(F32)
                    part = emu_contract(gblk, dt, c.stream, None, cm) if px.size else np.zeros((x.rows_p, ncol), F32)
                    stride = (x.rows if mutant == "slab_stride_rows" else x.rows_p) * k
                    base = slab0 * x.rows_p * k + rng_ * stride + k0
                    idx = base + np.arange(x.rows_p)[:, None] * k + np.arange(ncol)[None, :]
                    slab[idx] = part
                if "d" in x.outputs and px.size:      # ---- the grad_d tiles of this workgroup
                    vt = vpt[k0:k0 + ncol, r0v:r0v + x.rows_p]
                    part = emu_contract(gblk.T, vt.T, vstream, None, vm)
                    pv = px[valid]
                    idx = GD_PAD + pv[:, None] * k + k0 + np.arange(ncol)[None, :]
                    gdbuf[idx] = (gdbuf[idx] + part[valid]).astype(F32) if acc else part[valid]
    gd = gdbuf[GD_PAD:GD_PAD + p * k].reshape(p, k).copy()
    clean = bool((gdbuf[:GD_PAD] == SENTINEL).all() and (gdbuf[GD_PAD + p * k:] == SENTINEL).all())
    res = dict(clean=clean, vp=vp, vpt=vpt, plan=plan)
    if c.want_d:
        res["grad_d"] = res["grad_d_vpt"] = gd
    if c.want_v:
        res["grad_v"] = gv
        res["deferred"] = dict(is_slab=plan.nslabs > 0, nslabs=plan.nslabs, grad_v=gv)
    return res


def emu_gram(d, num_cu=256, mutant=None):
    """adil_gram: per workgroup the tiles of its range against themselves (both operands the same staged tile), a slab
    per workgroup, slab_sum.  mutants: emu_contract's | pix_tail_not_zeroed | skip_last_tile | slab_left_out | upper_only."""
    d = np.asarray(d, F32)
    p, k = d.shape
    nt, tpw, nwg = gram_plan(p, k, num_cu)
    cm = mutant if mutant in CONTRACT_MUTANTS else None
    slabs = np.full((nwg, k, k), np.nan, F32)
    for w in range(nwg):
        ta, tb = w * tpw, min(nt, (w + 1) * tpw)
        if mutant == "skip_last_tile" and w == nwg - 1:
            tb -= 1
        px = np.arange(ta * 32, max(tb, ta) * 32)
        dt = d[np.minimum(px, p - 1)]
        if mutant != "pix_tail_not_zeroed":
            dt = dt * (px < p)[:, None].astype(F32)
        slabs[w] = emu_contract(dt.T, dt, "f32", None, cm) if px.size else 0.0
    out = slab_sum(slabs, nwg - (1 if mutant == "slab_left_out" else 0))
    if mutant == "upper_only":
        out = np.triu(out)
    return out


def emu_rightmul(d, m, num_cu=256, mutant=None):
    """adil_dict_rightmul: 32-pixel blocks of D (K padded to a multiple of 16, tails zeroed) against the rows of M.
    mutants: emu_contract's | m_not_transposed | atom_tail_not_zeroed (BOTH staged operands keep the clamped loads) |
    skip_last_tile (the last block of the first workgroup's walk)."""
    d, m = np.asarray(d, F32), np.asarray(m, F32)
    p, k = d.shape
    kp = round_up(k, 16)
    cm = mutant if mutant in CONTRACT_MUTANTS else None
    cols = np.minimum(np.arange(kp), k - 1)
    keep = (np.arange(kp) < k).astype(F32) if mutant != "atom_tail_not_zeroed" else np.ones(kp, F32)
    mm = m if mutant == "m_not_transposed" else m.T
    out = emu_contract(d[:, cols] * keep[None, :], mm[cols] * keep[:, None], "f32", None, cm)
    if mutant == "skip_last_tile":
        nblocks, grid, walk = rightmul_plan(p, k, num_cu)
        last = (walk - 1) * grid
        out[32 * last:32 * last + 32] = np.nan
    return out


# ======================================================================================================= operand generators
class GradRow(NamedTuple):
    stream: str
    b: int
    p: int
    k: int
    wants: tuple = ("dv",)      # outputs asked for, per call: "dv", "d", "v"
    off: int = 0                # elements g sits past a 16-byte boundary
    big_p: bool = False         # P is raised by rule until the plan has tpw >= 2 (more tiles than workgroups)


def row_id(r):
    return f"grad-{r.stream}-B{r.b}-P{r.p}-K{r.k}-{'+'.join(r.wants)}" + (f"-off{r.off}" if r.off else "")


def resolve_row(r, num_cu):
    """big_p rows: P grows by its own value until every tile loop of the plan walks at least two tiles per workgroup."""
    if not r.big_p:
        return r
    p = r.p
    while True:
        pl = grad_plan(r.stream, r.b, p, r.k, "d" in r.wants[0], "v" in r.wants[0], True, num_cu)
        loops = [x for x in pl.kernels() if x.kernel != "grad_d_mfma" and x.fast]
        if loops and all(x.tpw >= 2 for x in loops):
            return r._replace(p=p)
        p += r.p


MID_NNZ = 12
GRIDS = {"f32": ("narrow", "mid", "wide_g", "wide_v", "wide_d"), "bf16": ("narrow", "mid")}
NARROW_INIT = 4096


def _halving(limit, top):
    """The largest 2^n - 1 <= top with (2^n - 1) <= limit."""
    m = top
    while m > 1 and m > limit:
        m //= 2
    return m


def _sparse_columns(rng, n, k, nnz):
    keep = np.zeros((n, k), bool)
    for j in range(k):
        keep[rng.permutation(n)[:nnz], j] = True
    return keep


def _one_per_column(rng, n, k, mag):
    a = np.zeros((n, k))
    a[rng.integers(0, n, size=k), np.arange(k)] = rng.choice([-1, 1], size=k) * mag
    return a


class GradOperands(NamedTuple):
    g: np.ndarray
    d: np.ndarray
    v: np.ndarray
    init: np.ndarray
    q_d: float
    q_v: float


def grad_operands(r, grid):
    """Operands of one row on one exact grid (module docstring), seeded from the row and the grid."""
    rng = np.random.default_rng(seed_of(f"{row_id(r)}-{grid}"))
    b, p, k = r.b, r.p, r.k
    init = np.zeros((p, k))
    if grid == "narrow":
        vmax = _halving((2 ** 24 - NARROW_INIT - 1) // (b * 127), 7)
        dmax = _halving((2 ** 24 - 1) // (p * 127), 127)
        g = C._ints(rng, -127, 127, (b, p)) * 2.0 ** -7
        v = C._ints(rng, -vmax, vmax, (b, k)) * 2.0 ** -7
        d = C._ints(rng, -dmax, dmax, (p, k)) * 2.0 ** -7
        init = C._ints(rng, -NARROW_INIT, NARROW_INIT, (p, k)) * 2.0 ** -14
        q_d = q_v = 2.0 ** -14
    elif grid == "mid":
        ncls = len(C.MID_CLASSES)
        cb = (np.arange(b) + int(rng.integers(0, ncls))) % ncls
        cp = (np.arange(p) + int(rng.integers(0, ncls))) % ncls
        g, v, d = np.zeros((b, p)), np.zeros((b, k)), np.zeros((p, k))
        for i, (a, cc) in enumerate(C.MID_CLASSES):
            rb, rp = np.flatnonzero(cb == i), np.flatnonzero(cp == i)
            g[np.ix_(rb, rp)] = C._exact_bits(rng, a, (rb.size, rp.size)) * 2.0 ** -a
            v[rb] = C._exact_bits(rng, cc, (rb.size, k)) * 2.0 ** (a - 23)
            d[rp] = C._exact_bits(rng, cc, (rp.size, k)) * 2.0 ** (a - 23)
        v = np.where(_sparse_columns(rng, b, k, MID_NNZ), v, 0.0)
        d = np.where(_sparse_columns(rng, p, k, MID_NNZ), d, 0.0)
        init = C._ints(rng, -2 ** 19, 2 ** 19, (p, k)) * 2.0 ** -23
        q_d = q_v = C.MID_Q
    elif grid == "wide_g":
        g = C._exact_bits(rng, 24, (b, p)) * 2.0 ** -24
        v = _one_per_column(rng, b, k, 2.0 ** -2)
        d = _one_per_column(rng, p, k, 2.0 ** -6)
        q_d, q_v = 2.0 ** -26, 2.0 ** -30
    elif grid == "wide_v":
        v = C._exact_bits(rng, 24, (b, k)) * 2.0 ** -29
        g = _one_per_column(rng, b, p, 2.0 ** -2)
        d = C._ints(rng, -127, 127, (p, k)) * 2.0 ** -7
        q_d, q_v = 2.0 ** -31, 2.0 ** -9
    elif grid == "wide_d":
        d = C._exact_bits(rng, 24, (p, k)) * 2.0 ** -24
        g = _one_per_column(rng, p, b, 2.0 ** -6).T
        v = C._ints(rng, -7, 7, (b, k)) * 2.0 ** -7
        q_d, q_v = 2.0 ** -13, 2.0 ** -30
    else:
        raise ValueError(grid)
    g = g.astype(F32)
    if r.stream == "bf16":
        g = rne_bf16(g)
    return GradOperands(g, d.astype(F32), v.astype(F32), init.astype(F32), q_d, q_v)


def assert_exact_premise(a64, b64, init64, q, what):
    """out = a b + init with a (M, n), b (n, N) in float64, as multiplied: every term a[i, j] b[j, l] is a multiple of q
    (per reduction index j the lowest set bits of column j of a and row j of b multiply to at least q), init is a
    multiple of q, and sum |terms| + |init| < 2^24 q.  Every partial sum, in any order, is then an fp32 number."""
    tq = low_quantum(a64, 0) * low_quantum(b64, 1)
    assert (tq >= q).all(), f"{what}: a product is not a multiple of q"
    s = np.abs(a64) @ np.abs(b64)
    ref = a64 @ b64
    if init64 is not None:
        assert np.array_equal(np.rint(init64 / q) * q, init64), f"{what}: init is not on the grid"
        s, ref = s + np.abs(init64), ref + init64
    assert float(s.max()) < 2.0 ** 24 * q, f"{what}: sum |terms| + |init| = {float(s.max())} >= 2^24 q"
    assert np.array_equal(np.rint(ref / q) * q, ref), what
    r32 = ref.astype(F32)
    assert np.array_equal(r32.astype(np.float64), ref), f"{what}: the reference is not an fp32 number"
    return r32


def grad_reference(r, grid):
    """(operands, want grad_d without init, want grad_d on init, want grad_v) of an exact row, premises asserted."""
    o = grad_operands(r, grid)
    what = f"{row_id(r)}-{grid}"
    g64 = o.g.astype(np.float64)
    v64, d64 = operands64(o.v, r.stream), operands64(o.d, r.stream)
    gd0 = assert_exact_premise(g64.T, v64, None, o.q_d, what + " grad_d")
    gd1 = assert_exact_premise(g64.T, v64, o.init.astype(np.float64), o.q_d, what + " grad_d + init")
    gv = assert_exact_premise(g64, d64, None, o.q_v, what + " grad_v")
    return o, gd0, gd1, gv


def grad_cases(r, o):
    """The calls of a row: per wanted output set, without and (where grad_d is asked for) with accumulation."""
    for w in r.wants:
        for acc in ((False, True) if "d" in w else (False,)):
            yield GradCase(f"{row_id(r)}-{w}{'-acc' if acc else ''}", o.g, o.d, o.v, r.stream, "d" in w, "v" in w,
                           o.init if acc else None, r.off)


def _compare(res, c, want_d, want_v, vp, vpt, plan, cmp):
    assert res["clean"], f"{c.name}: written outside grad_d"
    if c.want_d:
        cmp(res["grad_d"], want_d, f"{c.name}: grad_d")
        cmp(res["grad_d_vpt"], want_d, f"{c.name}: grad_d with vpt=")
    if c.want_v:
        cmp(res["grad_v"], want_v, f"{c.name}: grad_v")
        df = res["deferred"]
        assert df["is_slab"] == (plan.nchunks == 1), f"{c.name}: deferred grad_v is a SlabGrad iff the plan has one chunk"
        assert df["nslabs"] == plan.nslabs, f"{c.name}: nslabs {df['nslabs']} != plan {plan.nslabs}"
        cmp(df["grad_v"], want_v, f"{c.name}: deferred grad_v")
    assert_bits_equal(res["vp"], vp, f"{c.name}: vp")
    assert_bits_equal(res["vpt"], vpt, f"{c.name}: vpt")


def check_grad_exact(r, grid, run, num_cu=256):
    """run(case, plan) -> dict(grad_d, grad_d_vpt (the call with vpt= from pack_codes), grad_v, deferred = dict(is_slab,
    nslabs, grad_v summed by pack_codes), vp, vpt (as float32), clean).  Every output: bits of the reference."""
    o, gd0, gd1, gv = grad_reference(r, grid)
    vp, vpt = ref_pack(o.v, r.b, r.k, r.stream)
    for c in grad_cases(r, o):
        plan = case_plan(c, num_cu)
        bits = lambda got, want, what: assert_bits_equal(np.asarray(got, F32), want, what, ignore_zero_sign=True)
        _compare(run(c, plan), c, gd1 if c.init is not None else gd0, gv, vp, vpt, plan, bits)


def grad_bound(s, n, extra, stream):
    """|out - r| <= A = 2 (n + extra) 2^-24 S (+ 2^-23 S on fp32 streams), elementwise, r the float64 product of the
    operands AS MULTIPLIED and S = sum |terms| (+ |init|) over the n indices of the reduction axis.

    The outputs stay fp32, so there is no store rounding (u_T of contract_reference.gauss_bound is absent).
    Piece products are products of bf16 numbers: exact in fp32.  Each is accumulated in fp32: a chain of n additions of
    partial sums no larger than S loses at most n 2^-24 S to first order; the factor 2 covers the MFMA's internal sum of
    its 16 terms, whose order and intermediate rounding the ISA does not state.  `extra` counts the fp32 additions
    outside the MFMA chain: one per slab in slab_sum, one per row split met in LDS (at most 4) and one per row chunk
    accumulated into grad_d (plus the initial contents); the callers count slabs and chunks on the plan.
    fp32 streams: the lower piece products add roundings on partial sums no larger than S (the same A), and three of the
    nine piece products are never issued: |am bl| + |al bm| + |al bl| < 2^-24 |a b|; with the allowance of 2^-25 per
    operand of gauss_bound that is 2^-23 S.  bf16 streams: g is given in bf16 and the reference multiplies rne_bf16(V),
    rne_bf16(D) — the operand rounding is part of the reference, not of the error; the separate conversion of vpt by
    pack_codes is held to the bit against ref_pack."""
    a = 2.0 * (n + extra) * U24 * s
    return a + (2.0 ** -23 * s if stream == "f32" else 0.0)


def gauss_operands(r):
    rng = np.random.default_rng(seed_of(row_id(r) + "-gauss"))
    g = rng.standard_normal((r.b, r.p)).astype(F32)
    if r.stream == "bf16":
        g = rne_bf16(g)
    d = rng.uniform(-1, 1, (r.p, r.k)).astype(F32)
    v = (0.02 * rng.standard_normal((r.b, r.k))).astype(F32)
    init = (0.1 * rng.standard_normal((r.p, r.k))).astype(F32)
    return GradOperands(g, d, v, init, 0.0, 0.0)


def check_grad_gauss(r, run, num_cu=256):
    """Gaussian operands within grad_bound; run(case, plan) as in check_grad_exact, plus `again`: the outputs of a
    second identical call, which must have the same bits.  Returns the worst err / bound."""
    o = gauss_operands(r)
    vp, vpt = ref_pack(o.v, r.b, r.k, r.stream)
    worst = [0.0]
    for c in grad_cases(r, o):
        plan = case_plan(c, num_cu)
        gd, sd, gv, sv = ref_grad(o.g, o.d, o.v, r.stream, c.init)
        # additions outside the MFMA chains, counted on the plan: row chunks into grad_d (+ the initial contents, + at most 4
        # row splits met in LDS); the slabs of the widest reduction
        nch = len({x.r0 for x in plan.kernels() if "d" in x.outputs})
        nsl = max([x.nslabs for x in plan.launches if isinstance(x, Reduce)], default=0)
        bd = grad_bound(sd, r.b, nch + 1 + 4, r.stream)
        bv = grad_bound(sv, r.p, nsl, r.stream)

        def within(got, want, what):
            worst[0] = max(worst[0], assert_within(got, want, bd if want is gd else bv, what))
        res = run(c, plan)
        _compare(res, c, gd, gv, vp, vpt, plan, within)
        for key, first in (("grad_d", c.want_d), ("grad_v", c.want_v)):
            if first:
                assert_bits_equal(np.asarray(res["again"][key], F32), np.asarray(res[key], F32), f"{c.name}: second call, {key}")
    return worst[0]


# ============================================================================================================= Gram and D M^T
GRAM_K = (1, 17, 32, 33, 50, 64, 65, 100, 128)
GRAM_P = (32, 50, 432, 9605)
GRAM_GRIDS = ("narrow", "mid", "wide")
GRAM_MID_NNZ = 8


def gram_operands(p, k, grid):
    """narrow: D = i 2^-7 with |i| halved until P i^2 < 2^24, q = 2^-14.  mid: by pixel odd 9- or 10-bit integers
    2^-10 (a square has at most 20 bits: the diagonal allows no more) on at most 8 pixel rows shared by all columns, the
    first and the last pixel among them (every entry has up to 8 terms from different tiles), zero elsewhere, q = 2^-20.
    wide: even columns odd 24-bit integers 2^-24 on pairwise DISJOINT pixel sets, odd columns one +-2^-3 at a single
    pixel.  Returns (D, q, exact mask): entries between two wide columns are not exact (a 24-bit square has 48 bits);
    off the diagonal they are sums of zeros."""
    rng = np.random.default_rng(seed_of(f"gram-P{p}-K{k}-{grid}"))
    exact = np.ones((k, k), bool)
    if grid == "narrow":
        dmax = 127
        while p * dmax * dmax >= 2 ** 24:
            dmax //= 2
        return (C._ints(rng, -dmax, dmax, (p, k)) * 2.0 ** -7).astype(F32), 2.0 ** -14, exact
    if grid == "mid":
        bits = np.where(rng.random(p) < 0.5, 9, 10)
        d = np.zeros((p, k))
        for nb in (9, 10):
            rows = np.flatnonzero(bits == nb)
            d[rows] = C._exact_bits(rng, nb, (rows.size, k)) * 2.0 ** -10
        rows = np.unique(np.concatenate([[0, p - 1], rng.permutation(p)[:GRAM_MID_NNZ - 2]]))     # first, last (tail) pixel
        keep = np.zeros(p, bool)
        keep[rows] = True
        return np.where(keep[:, None], d, 0.0).astype(F32), 2.0 ** -20, exact
    d = np.zeros((p, k))
    wide = np.arange(0, k, 2)
    owner = rng.permutation(p) % wide.size if wide.size <= p else np.arange(p)      # pixel -> the wide column that owns it
    for i, col in enumerate(wide):
        rows = np.flatnonzero(owner == i)
        d[rows, col] = C._exact_bits(rng, 24, rows.size) * 2.0 ** -24
    for col in range(1, k, 2):
        d[int(rng.integers(0, p)), col] = float(rng.choice([-1, 1])) * 2.0 ** -3
    exact[np.ix_(wide, wide)] = False
    return d.astype(F32), 2.0 ** -27, exact


def check_gram(p, k, grid, run):
    """run(d) -> G (K, K).  Exact entries: bits, and bit-symmetric; entries between two wide columns: within grad_bound
    (their share is asserted to be at most a quarter of the matrix plus the diagonal)."""
    d, q, exact = gram_operands(p, k, grid)
    what = f"gram-P{p}-K{k}-{grid}"
    d64 = d.astype(np.float64)
    ref, s = ref_gram(d)
    if exact.all():
        want = assert_exact_premise(d64.T, d64, None, q, what)
    else:                                              # an exact entry has a one-hot column: at most one non-zero term
        assert (~exact).sum() <= k * k / 4 + k, f"{what}: too many inexact entries"
        onehot = np.flatnonzero(exact.all(0))
        assert ((d64[:, onehot] != 0).sum(0) <= 1).all(), f"{what}: a one-hot column has two entries"
        want = ref.astype(F32)
        assert np.array_equal(want.astype(np.float64)[exact], ref[exact]), f"{what}: an exact entry is not an fp32 number"
        off = ~exact & ~np.eye(k, dtype=bool)
        assert not s[off].any(), f"{what}: the wide columns overlap"
    got = np.asarray(run(d), F32)
    assert got.shape == (k, k)
    assert_bits_equal(np.where(exact, got, 0).astype(F32), np.where(exact, want, 0).astype(F32), what, ignore_zero_sign=True)
    assert_bits_equal(np.where(exact, got, 0).astype(F32), np.where(exact, got.T, 0).astype(F32), what + ": symmetry", ignore_zero_sign=True)
    worst = 0.0
    if not exact.all():
        n = int((d64 != 0).sum(0).max())
        worst = assert_within(np.where(exact, 0, got), np.where(exact, 0, ref), grad_bound(s, n, 2 * 256 + 2, "f32"), what + ": wide x wide")
    return worst


RIGHTMUL_GRIDS = ("narrow", "mid", "wide_d", "wide_m")


def rightmul_operands(p, k, grid):
    """D (P, K) and M (K, K) with the reduction along K: the synthesis grids of contract_reference with M in place of the
    codes (out = D M^T is V D^T transposed, B = K).  narrow: D = i 2^-7, M = j 2^-7, |i|, |j| <= 127 (K 127^2 < 2^24)."""
    rng = np.random.default_rng(seed_of(f"rightmul-P{p}-K{k}-{grid}"))
    if grid == "narrow":
        return (C._ints(rng, -127, 127, (p, k)) * 2.0 ** -7).astype(F32), (C._ints(rng, -127, 127, (k, k)) * 2.0 ** -7).astype(F32), 2.0 ** -14
    if grid == "mid":
        d, m = C.mid_dv(rng, p, k, k)
        return d, m, C.MID_Q
    d, m = C.wide_dv(rng, p, k, k, "d" if grid == "wide_d" else "v")
    return d, m, (2.0 ** -30 if grid == "wide_d" else 2.0 ** -31)


def check_rightmul(p, k, grid, run):
    """run(d, m) -> out (P, K): bits."""
    d, m, q = rightmul_operands(p, k, grid)
    what = f"rightmul-P{p}-K{k}-{grid}"
    want = assert_exact_premise(d.astype(np.float64), m.astype(np.float64).T, None, q, what)
    assert_bits_equal(np.asarray(run(d, m), F32), want, what, ignore_zero_sign=True)


def check_gram_gauss(p, k, run):
    rng = np.random.default_rng(seed_of(f"gram-P{p}-K{k}-gauss"))
    d = rng.uniform(-1, 1, (p, k)).astype(F32)
    ref, s = ref_gram(d)
    got = np.asarray(run(d), F32)
    assert_bits_equal(np.asarray(run(d), F32), got, f"gram-P{p}-K{k}: second call")
    return assert_within(got, ref, grad_bound(s, p, 2 * 256 + 2, "f32"), f"gram-P{p}-K{k}-gauss")


def check_rightmul_gauss(p, k, run):
    rng = np.random.default_rng(seed_of(f"rightmul-P{p}-K{k}-gauss"))
    d = rng.uniform(-1, 1, (p, k)).astype(F32)
    m = (rng.standard_normal((k, k)) / np.sqrt(k)).astype(F32)
    ref, s = ref_rightmul(d, m)
    got = np.asarray(run(d, m), F32)
    assert_bits_equal(np.asarray(run(d, m), F32), got, f"rightmul-P{p}-K{k}: second call")
    return assert_within(got, ref, grad_bound(s, k, 0, "f32"), f"rightmul-P{p}-K{k}-gauss")


# ===================================================================================================================== the rows
def _both(rows, streams=("f32", "bf16"), **kw):
    return [GradRow(s, b, p, k, **kw) for s in streams for b, p, k in rows]


BOUNDARY_K = (1, 16, 17, 32, 33, 64, 65, 96, 97, 127, 128)
ROWS = (
    # boundary values of K at (B, P) = (70, 72): both outputs, grad_d alone, grad_v alone
    _both([(70, 72, k) for k in BOUNDARY_K], wants=("dv", "d", "v"))
    # fused passes, K <= 64
    + _both([(33, 72, 10), (200, 72, 32), (300, 200, 17), (544, 72, 33)])
    + _both([(2048, 72, 50), (2049, 100, 50), (2049, 200, 10)], ("bf16",))
    + _both([(1024, 96, 64), (1030, 96, 50)], ("f32",))
    # bf16, K > 64: the atom-split pass, and past its limit
    + _both([(70, 72, 65), (300, 200, 97), (544, 72, 127), (2048, 72, 128), (2049, 72, 100)], ("bf16",))
    # fp32, K > 64
    + _both([(70, 96, 100), (600, 96, 128), (300, 72, 100)], ("f32",))
    # single outputs
    + _both([(70, 72, 100), (300, 72, 128)], ("bf16",), wants=("d",))
    + _both([(70, 200, 10), (70, 100, 50), (70, 50, 50)], wants=("d",))
    + _both([(70, 96, 10), (200, 96, 10), (300, 96, 50)], ("f32",), wants=("v",))
    + _both([(200, 72, 100), (600, 72, 113)], ("bf16",), wants=("v",))
    # g unaligned: the element-wise tiles only
    + [GradRow("f32", 70, 72, k, off=1) for k in (50, 100)] + [GradRow("bf16", 70, 72, k, off=2) for k in (50, 100)]
    # more tiles than workgroups: the prefetch and the buffer flip of every tile loop run
    + _both([(33, 19208, 50)], big_p=True) + _both([(33, 19208, 100)], ("bf16",), big_p=True)
    + _both([(33, 9600, 50), (33, 9600, 100)], ("f32",), big_p=True)
)
# Rows added so that the exact rows reach every instantiation (test_grad_reference_cpu.test_rows_reach_every_instantiation):
EXTRA_ROWS = (
    # grad_v_mfma<f32, 1 | 2, 8>: grad_v alone on fp32 with P % 32 != 0 and 128 < rows <= 256 (and a 4-wave last chunk)
    _both([(200, 72, 10), (300, 72, 50)], ("f32",), wants=("v",))
    # grad_v_mfma<bf16, 1 | 2, 4 | 8 | 16> and grad_d_mfma<bf16 | f32, 4, 1> with a slow tail, alone
    + _both([(600, 72, 10), (600, 200, 50)], ("bf16",), wants=("v",))
    + _both([(70, 72, 50), (200, 72, 50), (200, 72, 10)], ("bf16",), wants=("v",))
    # grad_v_f32<1 | 2, 4 | 8 | 16> beside the issue's rows
    + _both([(70, 96, 50), (200, 96, 50), (300, 96, 10)], ("f32",), wants=("v",))
    # grad_fused_mfma<bf16 | f32, 1 | 2, 4 | 8 (x RB), FAST, ACC>: every wave / row-block count with a fast tile and a tail
    + _both([(33, 72, 50), (200, 72, 10), (200, 72, 50), (300, 72, 10), (300, 72, 50)])
    # grad_fused_f32<1, 8>
    + _both([(70, 96, 10)], ("f32",))
    # launch_grad_d_lds with a fast tile
    + _both([(300, 200, 100)], ("bf16",), wants=("d",))
    # grad_d_mfma<f32, 2, 4> with a fast tile and a tail
    + _both([(70, 200, 100)], ("f32",), wants=("d",))
    # two tiles per workgroup in the single-output kernels: grad_v_mfma, the LDS grad_d route, grad_v_f32 without the split
    + [GradRow("bf16", 33, 19208, 50, ("v",), big_p=True), GradRow("bf16", 33, 19208, 100, ("d",), big_p=True),
       GradRow("f32", 33, 9600, 50, ("v",), big_p=True)]
)
ALL_ROWS = ROWS + EXTRA_ROWS

GAUSS_ROWS = (
    GradRow("bf16", 300, 200, 17), GradRow("f32", 300, 200, 17), GradRow("f32", 1024, 96, 64), GradRow("bf16", 544, 72, 127),
    GradRow("bf16", 2049, 72, 100), GradRow("f32", 600, 96, 128), GradRow("f32", 300, 72, 100), GradRow("bf16", 2049, 100, 50),
    GradRow("f32", 70, 200, 10, ("d",)), GradRow("f32", 300, 96, 50, ("v",)), GradRow("bf16", 33, 19208, 50, big_p=True),
)
GRAM_GAUSS = ((9605, 100),)
RIGHTMUL_GAUSS = ((432, 100),)
RIGHTMUL_P = (32, 50, 432)
RIGHTMUL_K = GRAM_K + (127,)
RIGHTMUL_BIG_K = (17, 100, 128)    # at the one P above 32 * 4 * (CU count)


def gram_big_p(num_cu):
    """The last P of GRAM_P, raised by 9600 until a workgroup walks two tiles (it is 9605 up to 300 CUs); 5 pixels of tail."""
    p = GRAM_P[-1]
    while gram_plan(p, 1, num_cu)[1] < 2:
        p += 9600
    return p


def rightmul_big_p(num_cu):
    """One P above 32 * 4 * (CU count): a workgroup walks two blocks; 5 pixels of tail."""
    return 32 * 4 * num_cu + 32 * 7 + 5
