"""float64 restatements of the frozen-classifier kernels (csrc/adil_convs.hip, csrc/adil_conv3x3.hip, csrc/adil_stem.hip, affine_act in
csrc/adil_update.hip), operand generators and two comparators.  Plain torch; works on the CPU and on a GPU.

The kernels multiply bf16 operands, accumulate in fp32 and round ONCE to bf16, to nearest even.  Two legs use that:

exact leg     Operands are small integers, BatchNorm scales are +-1/2, +-1, +-2 and shifts are integers.  Every product,
              every partial sum in ANY order and every epilogue value is then a multiple of a quantum q with magnitude
              below 2^23 q: exactly representable in fp32.  The one correct output is the RNE bf16 rounding of the exact
              value, so a kernel is compared BIT FOR BIT with the fp64 restatement, whatever its summation order.  The
              comparator first asserts the premise on the reference alone (sum |terms| = |A| @ |B| in fp64 < 2^23 q).
gaussian leg  N(0,1) operands, scales from [0.5, 1.5] with random signs.  Elementwise bound, derived, not measured:
                  |out - r| <= 2^-8 |r| + A (1 + 2^-8),   A = n 2^-24 S 2
              r = expected output in fp64 (after ReLU and masking), S = sum |terms| of that output, n = number of terms.
              A bounds fp32 accumulation in any order, the factor 2 covers the MFMA's undocumented internal summation; the
              kernel rounds a value within A of the exact one, so its half ulp is at most 2^-8 (|r| + A).  An output that
              is rounded twice on its way (the `xin` epilogue, the join's gres) is restated from the already rounded
              intermediate, so it too carries one rounding term.  Intermediate tensors the kernels round to bf16 before they feed a
              GEMM (the prologue x', the join's X0 and mid tensors) may legitimately differ by one bf16 step from the
              restatement's when the exact value sits next to a rounding boundary (an fp32 expression the compiler may
              or may not contract to an FMA; an accumulator that differs by its own error bound): both candidates are
              computed, the bound of the outputs they feed is widened by |candidate difference| @ |W|, and a mask taken
              from such a value accepts either candidate.  The allowance is added to A.  For the FMA candidates
              it is zero almost everywhere; for the mid tensors of the join and the `xin` epilogue a few percent of the
              elements carry it (the GPU test prints the fraction per row).  No element is excluded.

Every operation is written once over an `Arith`: fp64 with one matmul per GEMM is the reference; fp32 with the reduction
accumulated in 16- or 64-wide chunks, in tap order, is the CPU emulation of a kernel, which also takes the mutants of
tests/test_classifier_reference_cpu.py.  The 3x3 convolutions are written twice: padded slices (reference) and the
kernels' linear pixel shift with a validity mask (emulation)."""
import zlib
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
PW_BM = 128                      # pixel rows of a pointwise / join / stride-2 tile
CANARY = 4096.0                  # exact in bf16; no exact-leg or gaussian output reaches it by accident in a padded row
SCALES = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)


def bf16_rne(v):
    """bf16 rounding to nearest even of fp32-representable values, returned in v's dtype."""
    return v.float().bfloat16().to(v.dtype)


def bf16_trunc(v):
    return (v.float().contiguous().view(torch.int32) & -65536).view(F32).to(v.dtype)


def bits(t):
    """int16 view of bf16-representable values."""
    return t.bfloat16().contiguous().view(torch.int16)


class Arith:
    """dtype F64, chunk None: the reference.  dtype F32, chunk 16 / 64: the emulation of a kernel.  mut: mutant switches."""

    def __init__(self, dtype=F64, chunk=None, mut=()):
        self.dtype, self.chunk, self.mut = dtype, chunk, frozenset(mut)
        self.ref = chunk is None

    def mm(self, a, b):
        """a [M][K] . b [K][N]; an accumulator that starts at +0 (a zero result is +0, as in the MFMA)."""
        a, b = a.to(self.dtype), b.to(self.dtype)
        if self.chunk is None:
            return a @ b + 0.0
        acc = torch.zeros(a.shape[0], b.shape[1], dtype=self.dtype, device=a.device)
        for k0 in range(0, a.shape[1], self.chunk):
            acc = acc + a[:, k0:k0 + self.chunk] @ b[k0:k0 + self.chunk]
        return acc

    def f32(self, v):
        """A value the kernels hold in an fp32 register."""
        return v.float()

    def rnd(self, v):
        return bf16_trunc(v) if "trunc" in self.mut else bf16_rne(v)

    def pos(self, y):
        return y >= 0 if "ge_mask" in self.mut else y > 0

    def affine_rnd(self, x, s, b):
        """bf16(x * s + b) as the kernels form it in fp32, and |difference| to the other candidate (FMA or not)."""
        x32, s32, b32 = x.float(), s.float(), b.float()
        sep = self.rnd(x32 * s32 + b32)                                # two fp32 roundings
        if not self.ref:
            return sep.to(self.dtype), None
        fma = self.rnd((x.double() * s.double() + b.double()).float())  # exact sum, one fp32 rounding
        return fma.double(), (fma - sep).double().abs()

    def window_rnd(self, v, eps):
        """bf16(v) and how far bf16 of any value within eps of v can be from it."""
        r = self.rnd(v)
        if not self.ref or eps is None:
            return r, None
        return r, (bf16_rne((v + eps).float()) - bf16_rne((v - eps).float())).double().abs()


class Unrounded(Arith):
    """The reference with every rounding taken out: fp32 registers are fp64, `rnd` is the identity, no candidate differs.
    Each restatement is then the plain real-valued function it rounds (tests/resnet_tape.py holds a whole network's
    call sequence to the fp64 torch modules with it)."""

    def __init__(self, mut=()):
        super().__init__(F64, None, mut)

    def f32(self, v):
        return v.double()

    def rnd(self, v):
        return v

    def affine_rnd(self, x, s, b):
        return x.double() * s.double() + b.double(), None

    def window_rnd(self, v, eps):
        return v, (None if eps is None else torch.zeros_like(v))


class Out(NamedTuple):
    pre: torch.Tensor                      # the value before its last rounding
    S: Optional[torch.Tensor]              # sum |terms| of pre (reference only)
    n: int                                 # number of terms of pre
    q: float = 1.0                         # exact leg: pre and every partial sum are multiples of q
    relu: bool = False                     # ReLU after the rounding
    mask: Optional[torch.Tensor] = None    # keep-mask after the rounding (False -> +0)
    alt_mask: Optional[torch.Tensor] = None  # gaussian leg: the other candidate of `mask`
    widen: Optional[torch.Tensor] = None   # gaussian leg: allowance from rounded operands
    dtype: torch.dtype = BF16              # storage type of the output
    pre0: Optional[torch.Tensor] = None    # outputs rounded twice (`xin` epilogue): the value before the FIRST rounding;
                                           # `pre` is built from the rounded one, and in the exact leg its own rounding
                                           # is exact (a bf16 value times a power of two)


def finish(ar, o):
    """The output tensor (values, in the arithmetic's dtype) of an Out."""
    v = ar.rnd(o.pre) if o.dtype == BF16 else ar.f32(o.pre).to(o.pre.dtype)
    if o.relu:
        v = torch.where(v > 0, v, torch.zeros_like(v))
    if o.mask is not None:
        v = torch.where(o.mask, v, torch.zeros_like(v))
    return v


def acc_eps(S, n):
    return n * 2.0 ** -24 * S * 2


# ----------------------------------------------------------------------------------------------- pointwise convolution
def gather_rows(M, sub_w, sub_hw, device):
    """Row of the 2OH x 2OW input tensor that output pixel m = (n, oh, ow) of a stride-2 pointwise convolution reads."""
    m = torch.arange(M, device=device)
    n, r = m // sub_hw, m % sub_hw
    oh, ow = r // sub_w, r % sub_w
    return n * 4 * sub_hw + 2 * oh * 2 * sub_w + 2 * ow


def pw_fwd(ar, x, w, scale, shift, res=None, relu=1, pscale=None, pshift=None, sub_w=0, sub_hw=0, M=None):
    """y[M][N] = act((x'[M][K] . w[N][K]^T) * scale + shift (+ res)); x' = relu(bf16(x * pscale + pshift)) or x;
    stride 2: x' rows gathered from pixel (n, 2oh, 2ow)."""
    dt = ar.dtype
    M = x.shape[0] if M is None else M
    if sub_w:
        x = x[gather_rows(M, sub_w, sub_hw, x.device)]
    q, d0 = 1.0, None
    if pscale is not None:
        xp, d0 = ar.affine_rnd(x, pscale, pshift)
        xp = torch.where(xp > 0, xp, torch.zeros_like(xp))
        q = 0.5
    else:
        xp = x.to(dt)
    sc, sh = scale.to(dt), shift.to(dt)
    acc = ar.mm(xp, w.to(dt).t())
    pre = acc * sc + sh
    S = widen = None
    if ar.ref:
        S = (xp.abs() @ w.to(dt).abs().t()) * sc.abs() + sh.abs()
        if d0 is not None and bool(d0.any()):
            widen = (d0 @ w.to(dt).abs().t()) * sc.abs()
    if res is not None:
        pre = pre + res.to(dt)
        S = S + res.to(dt).abs() if ar.ref else None
    return {"y": Out(pre, S, x.shape[1] + 2, q * 0.5, relu=bool(relu), widen=widen)}


def up2(g3, M, sub_w, sub_hw, odd_pixel=False):
    """[M][N] zero-upsampled from g3 [M/4][N] on the stride-2 grid: pixel (n, h, w) gets g3[(n, h/2, w/2)] for even h, w."""
    out = torch.zeros(M, g3.shape[1], dtype=g3.dtype, device=g3.device)
    out[gather_rows(M // 4, sub_w, sub_hw, g3.device)] = g3
    if odd_pixel:                                                      # mutant: g3 also lands on an odd pixel
        out[1] = g3[0]
    return out


def pw_bwd(ar, g, wt, scale, y=None, g2=None, relu=1, xin=None, pscale=None, pshift=None, g3=None, sub_w=0, sub_hw=0,
           want_gres=True):
    """v = g (+ g2) (+ up2(g3)); gres = bf16(v) & mask; gz = bf16(v * scale) & mask; gx = gz . wt^T, wt [K][N];
    with xin: gx = bf16(bf16(gx) * pscale) where xin * pscale + pshift > 0, else +0.  v and gz are formed in fp32 in the
    kernel's order (no contraction can change them: the only product next to a sum is by 0 or 1)."""
    dt = ar.dtype
    M, N = g.shape
    v = ar.f32(g)
    S = g.to(dt).abs()
    if g2 is not None:
        v = v + ar.f32(g2)
        S = S + g2.to(dt).abs()
    if g3 is not None:
        u = up2(g3, M, sub_w, sub_hw, "g3_odd" in ar.mut)
        v = v + ar.f32(u)
        S = S + u.to(dt).abs()
    mask = ar.pos(y.to(dt)) if relu else None
    gz = ar.rnd(v * ar.f32(scale)).to(dt)
    if mask is not None:
        gz = torch.where(mask, gz, torch.zeros_like(gz))
    acc = ar.mm(gz, wt.to(dt).t())
    Sx = gz.abs() @ wt.to(dt).abs().t() if ar.ref else None
    outs = {}
    if want_gres:
        outs["gres"] = Out(v.to(dt), S, 3, 1.0, mask=mask)
    if xin is None:
        outs["gx"] = Out(acc, Sx, N, 0.5)
        return outs
    ps, pb = pscale.to(dt), pshift.to(dt)
    eps = acc_eps(Sx, N) if ar.ref else None
    gx1, d1 = ar.window_rnd(acc, eps)
    cond = ar.f32(xin) * ar.f32(pscale) + ar.f32(pshift) > 0           # separate fp32 roundings
    alt = None
    if ar.ref:
        alt = (xin.double() * ps + pb).float() > 0                     # contracted to an FMA
        Sx = Sx * ps.abs()
    widen = d1 * ps.abs() if d1 is not None and bool(d1.any()) else None
    outs["gx"] = Out(gx1 * ps, Sx, N + 1, 0.25, mask=cond, alt_mask=alt, widen=widen, pre0=acc)
    return outs


# ------------------------------------------------------------------------------------------------------ residual join
def join_fwd(ar, h2raw, pscale2, pshift2, w3, scale3, shift3, res, w1, scale1, shift1):
    """X0 = relu(bf16(h2raw * pscale2 + pshift2)); out = relu(bf16((X0 . w3^T) * scale3 + shift3 + res));
    h1 = relu(bf16((out . w1^T) * scale1 + shift1)).  w3 [C][W], w1 [W][C]."""
    dt = ar.dtype
    x0, d0 = ar.affine_rnd(h2raw, pscale2, pshift2)
    x0 = torch.where(x0 > 0, x0, torch.zeros_like(x0))
    s3, b3, s1, b1 = (t.to(dt) for t in (scale3, shift3, scale1, shift1))
    W3, W1 = w3.to(dt), w1.to(dt)
    pre_o = ar.mm(x0, W3.t()) * s3 + b3 + res.to(dt)
    So = wid_o = eps = None
    if ar.ref:
        So = (x0.abs() @ W3.abs().t()) * s3.abs() + b3.abs() + res.to(dt).abs()
        eps = acc_eps(So, W3.shape[1] + 2)
        if d0 is not None and bool(d0.any()):
            wid_o = (d0 @ W3.abs().t()) * s3.abs()
            eps = eps + wid_o
    mid, dm = ar.window_rnd(pre_o, eps)
    mid = torch.where(mid > 0, mid, torch.zeros_like(mid))
    pre_h = ar.mm(mid, W1.t()) * s1 + b1
    Sh = wid_h = None
    if ar.ref:
        Sh = (mid.abs() @ W1.abs().t()) * s1.abs() + b1.abs()
        if bool(dm.any()):
            wid_h = (dm @ W1.abs().t()) * s1.abs()
    return {"out": Out(pre_o, So, W3.shape[1] + 2, 0.25, relu=True, widen=wid_o),
            "h1": Out(pre_h, Sh, W1.shape[1] + 1, 0.125, relu=True, widen=wid_h)}


def join_bwd(ar, g_h1, h1, scale1, wt1, g_out, out, scale3, wt3, h2raw, pscale2, pshift2):
    """X0 = bf16(g_h1 * scale1) & [h1 > 0]; t = bf16(X0 . wt1^T); v = t + g_out; gres = bf16(v) & [out > 0];
    gz = bf16(v * scale3) & [out > 0]; gx = bf16(bf16(gz . wt3^T) * pscale2) where h2raw * pscale2 + pshift2 > 0.
    wt1 [C][W], wt3 [W][C]."""
    dt = ar.dtype
    m1, m3 = ar.pos(h1.to(dt)), ar.pos(out.to(dt))
    x0 = ar.rnd(ar.f32(g_h1) * ar.f32(scale1)).to(dt)
    x0 = torch.where(m1, x0, torch.zeros_like(x0))
    T1, T3 = wt1.to(dt), wt3.to(dt)
    acc_t = ar.mm(x0, T1.t())
    St = eps_t = None
    if ar.ref:
        St = x0.abs() @ T1.abs().t()
        eps_t = acc_eps(St, T1.shape[1])
    t, dt_ = ar.window_rnd(acc_t, eps_t)
    v = t + g_out.to(dt)                                               # exact in fp32: a bf16 value plus a bf16 value
    gz, dz = ar.window_rnd(v * scale3.to(dt), dt_ * scale3.to(dt).abs() if dt_ is not None else None)
    gz = torch.where(m3, gz, torch.zeros_like(gz))
    acc = ar.mm(gz, T3.t())
    ps, pb = pscale2.to(dt), pshift2.to(dt)
    Sv = Sx = wid_v = wid_x = None
    eps = None
    if ar.ref:
        Sv = t.abs() + g_out.to(dt).abs()
        wid_v = dt_ if bool(dt_.any()) else None
        Sx = gz.abs() @ T3.abs().t()
        eps = acc_eps(Sx, T3.shape[1])
        if bool(dz.any()):
            eps = eps + torch.where(m3, dz, torch.zeros_like(dz)) @ T3.abs().t()
    gx1, d1 = ar.window_rnd(acc, eps)
    cond = ar.f32(h2raw) * ar.f32(pscale2) + ar.f32(pshift2) > 0
    alt = None
    if ar.ref:
        alt = (h2raw.double() * ps + pb).float() > 0
        wid_x = (d1 + eps - acc_eps(Sx, T3.shape[1])) * ps.abs()
        Sx = Sx * ps.abs()
    return {"_t": Out(acc_t, St, T1.shape[1], 0.5),
            "gres": Out(v, Sv, 2, 0.5, mask=m3, widen=wid_v),
            "gx": Out(gx1 * ps, Sx, T3.shape[1] + 1, 0.125, mask=cond, alt_mask=alt, widen=wid_x,
                      pre0=acc)}


# ------------------------------------------------------------------------------------------------------ 3x3 convolutions
def _taps_linear(ar, x, H, W):
    """The kernels' formulation: pixels in linear order, tap (kh, kw) reads row m + (kh-1) W + (kw-1), masked where it
    leaves the image.  Mutants drop one side of the mask."""
    B = x.shape[0]
    M = B * H * W
    m = torch.arange(M, device=x.device)
    ww, hh = m % W, (m // W) % H
    xs = x.reshape(M, -1)
    for kh in range(3):
        for kw in range(3):
            ok = (hh + kh - 1 < H) & (ww + kw - 1 < W)
            if "no_wmask" not in ar.mut:
                ok &= ww + kw - 1 >= 0
            if "no_hmask" not in ar.mut:
                ok &= hh + kh - 1 >= 0
            rows = torch.roll(xs, -((kh - 1) * W + (kw - 1)), 0)
            yield kh, kw, torch.where(ok[:, None], rows, torch.zeros_like(rows))


def conv3x3(ar, x, w):
    """y[b][h][w][n] = sum x[b][h+kh-1][w+kw-1][c] w[n][c][kh][kw], zero padded.  x [B][H][W][C], w [N][C][3][3]."""
    dt = ar.dtype
    B, H, W, C = x.shape
    N = w.shape[0]
    wd = w.to(dt)
    if not ar.ref:
        acc = torch.zeros(B * H * W, N, dtype=dt, device=x.device)
        for kh, kw, rows in _taps_linear(ar, x.to(dt), H, W):
            acc = acc + ar.mm(rows, wd[:, :, kh, kw].t())
        return {"y": Out(acc.reshape(B, H, W, N), None, 9 * C)}
    xp = F.pad(x.to(dt), (0, 0, 1, 1, 1, 1))
    acc = torch.zeros(B * H * W, N, dtype=dt, device=x.device)
    S = torch.zeros_like(acc)
    for kh in range(3):
        for kw in range(3):
            rows = xp[:, kh:kh + H, kw:kw + W].reshape(-1, C)
            acc += rows @ wd[:, :, kh, kw].t()
            S += rows.abs() @ wd[:, :, kh, kw].abs().t()
    return {"y": Out(acc.reshape(B, H, W, N) + 0.0, S.reshape(B, H, W, N), 9 * C)}


def conv3x3_bwd(ar, g, w):
    """Input gradient of conv3x3: gx[b][h][w][c] = sum g[b][h+1-kh][w+1-kw][n] w[n][c][kh][kw].  g [B][H][W][N]."""
    return {"gx": conv3x3(ar, g, w.flip(2, 3).transpose(0, 1))["y"]}


def pack_taps(w):
    """[N][C][3][3] -> wp [N][9][C], tap kh*3+kw."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1]).contiguous()


def pack_taps_flipped(w):
    """[N][C][3][3] -> wp' [C][9][N] = w[n][c][2-kh][2-kw]: conv3x3 on it is the input gradient."""
    return pack_taps(w.flip(2, 3).transpose(0, 1))


def pack_taps_bwd_s2(w):
    """[N][C][3][3] -> wp_bwd [C][9][N], taps NOT flipped."""
    return pack_taps(w.transpose(0, 1))


def conv3x3_s2_fwd(ar, x, w):
    """y[b][i][j][n] = sum x[b][2i-1+kh][2j-1+kw][c] w[n][c][kh][kw].  x [B][H][W][C], H and W even."""
    dt = ar.dtype
    B, H, W, C = x.shape
    N, OH, OW = w.shape[0], H // 2, W // 2
    wd = w.to(dt)
    xp = F.pad(x.to(dt), (0, 0, 1, 1, 1, 1))
    acc = torch.zeros(B * OH * OW, N, dtype=dt, device=x.device)
    S = torch.zeros_like(acc) if ar.ref else None
    for kh in range(3):
        for kw in range(3):
            rows = xp[:, kh:kh + H:2, kw:kw + W:2].reshape(-1, C)
            if "no_wmask" in ar.mut and kw == 0:                      # mutant: column -1 reads the previous pixel
                rows = torch.roll(x.to(dt).reshape(-1, C), 1, 0).reshape(B, H, W, C)
                rows = F.pad(rows, (0, 0, 0, 0, 1, 1))[:, kh:kh + H:2, 0:W:2].reshape(-1, C)
            acc = acc + ar.mm(rows, wd[:, :, kh, kw].t())
            if ar.ref:
                S += rows.abs() @ wd[:, :, kh, kw].abs().t()
    return {"y": Out(acc.reshape(B, OH, OW, N), None if S is None else S.reshape(B, OH, OW, N), 9 * C)}


def conv3x3_s2_bwd(ar, g, w, H, W):
    """gx[b][h][w][c] = sum g[b][(h+1-kh)/2][(w+1-kw)/2][n] w[n][c][kh][kw] over integral, in-range quotients.
    g [B][OH][OW][N]; every tap's product [B][OH][OW][C] is added at input pixels (2i-1+kh, 2j-1+kw)."""
    dt = ar.dtype
    B, OH, OW, N = g.shape
    C = w.shape[1]
    wd = w.to(dt)
    acc = torch.zeros(B, H + 2, W + 2, C, dtype=dt, device=g.device)
    S = torch.zeros_like(acc) if ar.ref else None
    gs = g.to(dt).reshape(-1, N)
    for kh in range(3):
        for kw in range(3):
            t = ar.mm(gs, wd[:, :, kh, kw]).reshape(B, OH, OW, C)
            acc[:, kh:kh + H:2, kw:kw + W:2] += t
            if ar.ref:
                S[:, kh:kh + H:2, kw:kw + W:2] += (gs.abs() @ wd[:, :, kh, kw].abs()).reshape(B, OH, OW, C)
    if "no_hmask" in ar.mut:                                           # mutant: row -1 of an image is the previous image's last row
        acc[:-1, H] += acc[1:, 0]
    crop = lambda a: a[:, 1:H + 1, 1:W + 1].contiguous()
    return {"gx": Out(crop(acc) + 0.0, None if S is None else crop(S), 4 * N)}


# ---------------------------------------------------------------------------------------------------------------- stem
def pack_stem_fwd(w):
    """[64][3][7][7] -> w_fwd [64][7][8][4] = w[co][ci][kh][kw] at [co][kh][kw][ci], zero for kw = 7 / ci = 3."""
    out = torch.zeros(64, 7, 8, 4, dtype=w.dtype, device=w.device)
    out[:, :, :7, :3] = w.permute(0, 2, 3, 1)
    return out.contiguous()


def pack_stem_bwd(w):
    """[64][3][7][7] -> w_bwd [4][49][64] = w[co][ci][kh][kw] at [ci][kh*7+kw][co], zero for ci = 3."""
    out = torch.zeros(4, 49, 64, dtype=w.dtype, device=w.device)
    out[:3] = w.permute(1, 2, 3, 0).reshape(3, 49, 64)
    return out.contiguous()


def stem_fwd(ar, x, w, mean, inv_std, scale, shift):
    """y1 = relu(bf16(conv7x7/2(bf16((x - mean) * inv_std), zero padded) * scale + shift)), NHWC.  x [B][3][H][W] fp32
    or bf16, w [64][3][7][7].  (x - mean) * inv_std is two fp32 operations no contraction can merge."""
    dt = ar.dtype
    B, _, H, W = x.shape
    OH, OW = H // 2, W // 2
    mean = ar.f32(torch.tensor(mean, dtype=F64, device=x.device)).view(1, 3, 1, 1)     # fp32 arguments (the doubles over `Unrounded`)
    istd = ar.f32(torch.tensor(inv_std, dtype=F64, device=x.device)).view(1, 3, 1, 1)
    xn = ar.rnd((ar.f32(x) - mean) * istd).to(dt)
    cols = F.unfold(xn, 7, padding=3, stride=2)                        # [B][3*49][OH*OW], rows (ci, kh, kw)
    cols = cols.view(B, 3, 49, OH * OW).permute(0, 3, 2, 1).reshape(B * OH * OW, 147)     # (kh, kw, ci): the kernel's K order
    wk = w.to(dt).permute(0, 2, 3, 1).reshape(64, 147)
    sc, sh = scale.to(dt), shift.to(dt)
    pre = ar.mm(cols, wk.t()) * sc + sh
    S = (cols.abs() @ wk.abs().t()) * sc.abs() + sh.abs() if ar.ref else None
    return {"y": Out(pre.reshape(B, OH, OW, 64), None if S is None else S.reshape(B, OH, OW, 64), 148, 0.25, relu=True)}


def stem_bwd(ar, gy, w, inv_std, H, W, out_dtype):
    """gx[b][ci][ih][iw] = inv_std[ci] * sum gy[b][(ih+3-kh)/2][(iw+3-kw)/2][co] w[co][ci][kh][kw].  gy [B][OH][OW][64]."""
    dt = ar.dtype
    B, OH, OW, _ = gy.shape
    wk = w.to(dt).reshape(64, 147)                                     # columns (ci, kh, kw): F.fold's order
    gs = gy.to(dt).reshape(B, OH * OW, 64)
    istd = ar.f32(torch.tensor(inv_std, dtype=F64, device=gy.device)).to(dt).view(1, 3, 1, 1)   # the kernel takes fp32 arguments
    cols = ar.mm(gs.reshape(-1, 64), wk).reshape(B, OH * OW, 147).transpose(1, 2)
    acc = F.fold(cols, (H, W), 7, padding=3, stride=2) + 0.0
    S = None
    if ar.ref:
        S = F.fold((gs.reshape(-1, 64).abs() @ wk.abs()).reshape(B, OH * OW, 147).transpose(1, 2), (H, W), 7, padding=3,
                   stride=2) * istd
    return {"gx": Out(acc * istd, S, 64 * 16 + 1, 2.0 ** -4, dtype=out_dtype)}


# ---------------------------------------------------------------------------------------------------------- affine_act
def _channel(t, n, C, inner):
    return t[(torch.arange(n, device=t.device) // inner) % C]


def affine_act_fwd(ar, x, scale, shift, res, C, inner, relu, dtype):
    """y = act(fma(x, scale[c], shift[c]) (+ res)), channel of flat element i = (i / inner) % C."""
    dt = ar.dtype
    n = x.numel()
    sc, sh = _channel(scale, n, C, inner).to(dt), _channel(shift, n, C, inner).to(dt)
    xv = x.to(dt).flatten()
    if ar.ref:
        pre = xv * sc + sh
        S = xv.abs() * sc.abs() + sh.abs()
    else:
        pre = (xv.double() * sc.double() + sh.double()).float()         # fmaf: one rounding
        S = None
    if res is not None:
        pre = pre + res.to(dt).flatten()
        S = S + res.to(dt).flatten().abs() if ar.ref else None
    return {"y": Out(pre, S, 3, 0.5, relu=bool(relu), dtype=dtype)}


def affine_act_bwd(ar, g, y, scale, C, inner, relu, dtype, want_gres=True):
    """gres = g where y > 0, else +0; gx = gres * scale[c] (so a masked element is -0 under a negative scale, as in the
    kernel, which multiplies after masking)."""
    dt = ar.dtype
    n = g.numel()
    sc = _channel(scale, n, C, inner).to(dt)
    gv = g.to(dt).flatten()
    if relu:
        gv = torch.where(ar.pos(y.to(dt).flatten()), gv, torch.zeros_like(gv))
    outs = {"gx": Out(gv * sc, gv.abs() * sc.abs(), 1, 0.25, dtype=dtype)}
    if want_gres:
        outs["gres"] = Out(gv, gv.abs(), 1, 1.0, dtype=dtype)
    return outs


# ---------------------------------------------------------------------------------------------------------- operands
def rng(name, leg):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(f"{name}/{leg}".encode()))
    return g


class Gen:
    """Operand generator of one leg, on the CPU (the GPU tests copy the very same operands to the device)."""

    def __init__(self, name, leg):
        self.exact, self.g = leg == "exact", rng(name, leg)

    def act(self, *shape, amp=8):
        """bf16 activations / gradients: integers in [-amp, amp], or N(0, 1)."""
        if self.exact:
            return torch.randint(-amp, amp + 1, shape, generator=self.g).to(BF16)
        return torch.randn(shape, generator=self.g).to(BF16)

    def relu_out(self, *shape, amp=3):
        """What a mask [y > 0] is taken from: positive, +0 and (beyond what a ReLU emits, to test the mask on them too)
        negative values; no negative zero, which the kernels' callers must not pass."""
        if self.exact:
            return torch.randint(-2, amp + 1, shape, generator=self.g).to(BF16)
        y = torch.randn(shape, generator=self.g)
        return torch.where(torch.rand(shape, generator=self.g) < 0.25, torch.zeros(()), y).to(BF16) + 0.0

    def weight(self, *shape, amp=4, fan_in=None):
        if self.exact:
            return torch.randint(-amp, amp + 1, shape, generator=self.g).to(BF16)
        return (torch.randn(shape, generator=self.g) * (fan_in or shape[-1]) ** -0.5).to(BF16)

    def scale(self, n):
        """BatchNorm scale: +-1/2, +-1, +-2, or [0.5, 1.5] with a random sign (pretrained gammas are of both signs)."""
        if self.exact:
            return torch.tensor(SCALES)[torch.randint(0, len(SCALES), (n,), generator=self.g)]
        sign = torch.randint(0, 2, (n,), generator=self.g).float() * 2 - 1
        return (0.5 + torch.rand(n, generator=self.g)) * sign

    def shift(self, n, amp=8):
        if self.exact:
            return torch.randint(-amp, amp + 1, (n,), generator=self.g).float()
        return torch.randn(n, generator=self.g) * 0.5


# ---------------------------------------------------------------------------------------------------------- comparators
def tile_report(idx, shape, tile, bn, MT, NT):
    """(row, channel, row mod tile, channel mod BN, workgroup under the plain map, under the XCD swizzle) of flat index."""
    ch = int(idx % shape[-1])
    row = int(idx // shape[-1])
    if not tile:
        return f"(flat {int(idx)})"
    mt, nt = row // tile, ch // max(bn, 1)
    plain = mt * NT + nt
    swz = ((mt // 8) * NT + nt) * 8 + mt % 8
    return (f"(row {row}, channel {ch}, row mod {tile} = {row % tile}, channel mod {bn} = {ch % bn}, "
            f"workgroup {plain} plain / {swz} swizzled of {MT} x {NT})")


def assert_premise(name, o):
    """Exact leg, on the reference alone: every partial sum of `pre` is a multiple of q below 2^23 q."""
    worst = float((o.S / o.q).max())
    assert worst < 2.0 ** 23, f"{name}: sum |terms| = {worst:.0f} quanta >= 2^23: the exact leg's premise fails"
    k = o.pre / o.q
    assert bool((k == k.round()).all()), f"{name}: the reference is not a multiple of its quantum {o.q}"


def compare_exact(name, got, o, geom=None):
    """got: the kernel's (or emulation's) tensor; o: the reference Out.  Returns the mismatch count (raises if > 0)."""
    assert_premise(name, o)
    want = finish(Arith(), o)
    got = got.reshape(want.shape)
    if o.dtype == BF16:
        a, b = bits(got), bits(want)
    else:
        a, b = got.float().contiguous().view(torch.int32), want.float().contiguous().view(torch.int32)
    if torch.equal(a, b):
        return 0
    bad = (a != b).flatten()
    first = int(bad.nonzero()[0])
    where = tile_report(first, want.shape, *(geom or (0, 0, 0, 0)))
    raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} outputs differ in bits; first at {where}: got "
                         f"{float(got.flatten()[first])}, want {float(want.flatten()[first])} (exact {float(o.pre.flatten()[first])})")


def gaussian_bound(o, r):
    """A = n 2^-24 S 2 (+ the rounded-operand allowance) bounds how far the kernel's value before its bf16 rounding is
    from the fp64 value; the rounding adds at most half an ulp of that value, 2^-8 (|r| + A).  r is the expected OUTPUT:
    after ReLU and masking, so a clipped or masked element (r = 0) is allowed the accumulation term only.  fp32 outputs
    are not rounded to bf16: A alone."""
    a = acc_eps(o.S, o.n)
    if o.widen is not None:
        a = a + o.widen
    return ((2.0 ** -8 * (r.abs() + a) if o.dtype == BF16 else 0.0) + a).clamp_min(2.0 ** -126)


def gaussian_ratio(got, o):
    """max over elements of |got - r| / bound with bound = 2^-8 |r| + A (1 + 2^-8), A = n 2^-24 S 2 + allowance; where a
    mask has two candidates, the better of the two."""
    def ratio(mask):
        r = o.pre.clamp_min(0) if o.relu else o.pre
        if mask is not None:
            r = torch.where(mask, r, torch.zeros_like(r))
        return (got.reshape(r.shape).double() - r).abs() / gaussian_bound(o, r)

    q = ratio(o.mask)
    if o.alt_mask is not None:
        q = torch.minimum(q, ratio(o.alt_mask))
    return float(q.max())


def widened_fraction(o):
    """Fraction of the elements of an output whose gaussian bound carries a rounded-operand allowance."""
    return 0.0 if o.widen is None else float((o.widen > 0).double().mean())


def stats(o):
    """(fraction nonzero, fraction really rounded, fraction exact ties) of an exact-leg reference output."""
    want = finish(Arith(), o)
    nz = float((want != 0).double().mean())
    if o.dtype != BF16:
        return nz, 0.0, 0.0
    pre = o.pre if o.pre0 is None else o.pre0
    lo = bf16_trunc(pre)                                               # towards zero: the bottom of the value's bf16 step
    rounded = lo != pre
    a = lo.abs().clamp_min(2.0 ** -126)
    ulp = 2.0 ** (torch.floor(torch.log2(a)) - 7)
    tie = rounded & ((pre - lo).abs() * 2 == ulp)
    return nz, float(rounded.double().mean()), float(tie.double().mean())


# --------------------------------------------------------------------------------------------------------------- routes
class Route(NamedTuple):
    family: str       # pw_fwd pw_bwd join_fwd join_bwd conv3x3 conv3x3_bwd s2_fwd s2_bwd stem_fwd stem_bwd act_fwd act_bwd
    branch: str       # the launcher branch / kernel instantiation the row is meant to reach
    cfg: dict

    @property
    def name(self):
        return self.family + "-" + "-".join(f"{k}{_short(v)}" for k, v in self.cfg.items() if v not in (None, False, 0))


def _short(v):
    if v is True:
        return ""
    if isinstance(v, (tuple, list)):
        return "x".join(str(i) for i in v)
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    return str(v)


def geometry(r):
    """(tile rows, BN, MT, NT) of the kernel a row launches; (0, 0, 0, 0) where no tile map exists."""
    f, c = r.family, r.cfg
    if f in ("pw_fwd", "pw_bwd"):
        n = c["N"] if f == "pw_fwd" else c["K"]
        bn = 128 if n % 128 == 0 else 64
        return PW_BM, bn, -(-c["M"] // PW_BM), n // bn
    if f in ("join_fwd", "join_bwd"):
        return PW_BM, 64, -(-c["M"] // PW_BM), 1
    if f in ("conv3x3", "conv3x3_bwd"):
        n = c["N"] if f == "conv3x3" else c["C"]
        bn, tile = (128, 128) if n % 128 == 0 else (64, 256)
        return tile, bn, -(-c["B"] * c["H"] * c["W"] // tile), n // bn
    if f in ("s2_fwd", "s2_bwd"):
        n = c["N"] if f == "s2_fwd" else c["C"]
        bn = 128 if n % 128 == 0 else 64
        return PW_BM, bn, -(-c["B"] * c["H"] * c["W"] // 4 // PW_BM), n // bn
    return 0, 0, 0, 0


def operands(r, leg):
    """The operands of a row for one leg: CPU tensors in the kernels' storage types, keyed as `evaluate` takes them."""
    f, c, G = r.family, r.cfg, Gen(r.name, leg)
    ex = leg == "exact"
    if f == "pw_fwd":
        M, K, N = c["M"], c["K"], c["N"]
        sub = c.get("sub")
        o = dict(x=G.act(4 * M if sub else M, K), w=G.weight(N, K), scale=G.scale(N), shift=G.shift(N),
                 res=G.act(M, N) if c.get("res") else None, relu=c.get("relu", 1),
                 pscale=G.scale(K) if c.get("pro") else None, pshift=G.shift(K) if c.get("pro") else None,
                 sub_w=sub[1] if sub else 0, sub_hw=sub[0] * sub[1] if sub else 0, M=M)
        if c.get("zeros"):            # exact zeros in the pre-activation, of both signs: zero accumulators, +-0 shifts
            o["x"][::3] = 0
            o["shift"][::2] = -0.0
            o["shift"][1::4] = 0.0
        return o
    if f == "pw_bwd":
        M, K, N = c["M"], c["K"], c["N"]
        sub = c.get("g3")
        relu = c.get("relu", 1)
        return dict(g=G.act(M, N, amp=4), wt=G.weight(K, N), scale=G.scale(N), y=G.relu_out(M, N) if relu else None,
                    g2=G.act(M, N, amp=4) if c.get("g2") else None, relu=relu,
                    xin=G.act(M, K) if c.get("xin") else None, pscale=G.scale(K) if c.get("xin") else None,
                    pshift=G.shift(K) if c.get("xin") else None, g3=G.act(M // 4, N, amp=4) if sub else None,
                    sub_w=sub[1] if sub else 0, sub_hw=sub[0] * sub[1] if sub else 0, want_gres=bool(c.get("gres")))
    if f == "join_fwd":
        M, W = c["M"], c["W"]
        C = 4 * W
        return dict(h2raw=G.act(M, W, amp=4), pscale2=G.scale(W), pshift2=G.shift(W, 4), w3=G.weight(C, W, amp=2),
                    scale3=G.scale(C), shift3=G.shift(C), res=G.act(M, C), w1=G.weight(W, C, amp=2), scale1=G.scale(W),
                    shift1=G.shift(W))
    if f == "join_bwd":
        M, W = c["M"], c["W"]
        C = 4 * W
        return dict(g_h1=G.act(M, W, amp=4), h1=G.relu_out(M, W), scale1=G.scale(W), wt1=G.weight(C, W, amp=2),
                    g_out=G.act(M, C, amp=4), out=G.relu_out(M, C), scale3=G.scale(C), wt3=G.weight(W, C, amp=2),
                    h2raw=G.act(M, W, amp=4), pscale2=G.scale(W), pshift2=G.shift(W, 4))
    if f in ("conv3x3", "s2_fwd"):
        return dict(x=G.act(c["B"], c["H"], c["W"], c["C"]), w=G.weight(c["N"], c["C"], 3, 3, fan_in=9 * c["C"]))
    if f == "conv3x3_bwd":
        return dict(g=G.act(c["B"], c["H"], c["W"], c["N"]), w=G.weight(c["N"], c["C"], 3, 3, fan_in=9 * c["N"]))
    if f == "s2_bwd":
        return dict(g=G.act(c["B"], c["H"] // 2, c["W"] // 2, c["N"]), w=G.weight(c["N"], c["C"], 3, 3, fan_in=4 * c["N"]),
                    H=c["H"], W=c["W"])
    if f == "stem_fwd":
        x = G.act(c["B"], 3, c["H"], c["W"], amp=16) if ex else torch.rand(c["B"], 3, c["H"], c["W"], generator=G.g)
        mean = (0.0, 2.0, -3.0) if ex else (0.485, 0.456, 0.406)
        istd = (1.0, 0.5, 2.0) if ex else (1 / 0.229, 1 / 0.224, 1 / 0.225)
        return dict(x=x.to(c["dtype"]), w=G.weight(64, 3, 7, 7, fan_in=147), mean=mean, inv_std=istd, scale=G.scale(64),
                    shift=G.shift(64))
    if f == "stem_bwd":
        istd = (1.0, 0.5, 2.0) if ex else (1 / 0.229, 1 / 0.224, 1 / 0.225)
        return dict(gy=G.act(c["B"], c["H"] // 2, c["W"] // 2, 64), w=G.weight(64, 3, 7, 7, fan_in=64 * 12), inv_std=istd,
                    H=c["H"], W=c["W"], out_dtype=c["dtype"])
    if f in ("act_fwd", "act_bwd"):
        n, C, inner, dt = c["n"], c["C"], c["inner"], c["dtype"]

        def val(amp=15):              # exact leg: a * 2^e, |a| <= amp: bf16 values whose sums need rounding
            if not ex:
                return torch.randn(n, generator=G.g).to(dt)
            a = torch.randint(-amp, amp + 1, (n,), generator=G.g).float()
            return (a * 2.0 ** torch.randint(0, 7, (n,), generator=G.g).float()).to(dt)
        if f == "act_fwd":
            return dict(x=val(), scale=G.scale(C), shift=G.shift(C), res=val() if c.get("res") else None, C=C, inner=inner,
                        relu=c.get("relu", 1), dtype=dt)
        relu = c.get("relu", 1)
        scale = G.scale(C)
        if ex:                        # g * 2^k never needs rounding: 8-bit g and half the scales times 1.5, still one exact
            scale = scale * torch.where(torch.arange(C) % 2 == 0, 1.5, 1.0)      # fp32 product, rounded once to bf16
        return dict(g=val(255), y=G.relu_out(n).to(dt) if relu else None, scale=scale, C=C, inner=inner, relu=relu, dtype=dt,
                    want_gres=bool(c.get("gres")))
    raise KeyError(f)


OPS = {"pw_fwd": pw_fwd, "pw_bwd": pw_bwd, "join_fwd": join_fwd, "join_bwd": join_bwd, "conv3x3": conv3x3,
       "conv3x3_bwd": conv3x3_bwd, "s2_fwd": conv3x3_s2_fwd, "s2_bwd": conv3x3_s2_bwd, "stem_fwd": stem_fwd,
       "stem_bwd": stem_bwd, "act_fwd": affine_act_fwd, "act_bwd": affine_act_bwd}


def evaluate(r, ar, o):
    """The Outs of a row under an arithmetic (reference or emulation)."""
    return OPS[r.family](ar, **o)


# ------------------------------------------------------------------------------------------------- launch signatures
RECORDED_PREFIXES = ("adil_pw_", "adil_conv3x3", "adil_stem_conv", "adil_affine_act_")


def _set(a):
    return bool(getattr(a, "value", a))


def _int(a):
    return int(getattr(a, "value", a))


def _swz(m, tile):
    return (-(-m // tile)) % 8 == 0


def call_signature(entry, a):
    """What decides the launcher branch of one C ABI call of the classifier kernels, from its argument list: entry, the
    channel counts, which optional pointers are set, relu, stride-2 gather, the BN / BO tile, and MT mod 8 == 0 (the XCD
    swizzle)."""
    if entry == "adil_pw_conv_fwd":          # x w scale shift res y M K N relu pscale pshift sub_w sub_hw
        M, K, N = _int(a[6]), _int(a[7]), _int(a[8])
        return (entry, f"K={K}", f"N={N}", f"res={int(_set(a[4]))}", f"pro={int(_set(a[10]))}", f"relu={_int(a[9])}",
                f"gather={int(_int(a[12]) > 0)}", f"BN={128 if N % 128 == 0 else 64}", f"swizzle={int(_swz(M, PW_BM))}")
    if entry == "adil_pw_conv_bwd":          # g g2 y scale wt gx gres M K N relu xin pscale pshift g3 sub_w sub_hw
        M, K, N = _int(a[7]), _int(a[8]), _int(a[9])
        return (entry, f"K={K}", f"N={N}", f"g2={int(_set(a[1]))}", f"gres={int(_set(a[6]))}", f"xin={int(_set(a[11]))}",
                f"g3={int(_set(a[14]))}", f"relu={_int(a[10])}", f"BO={128 if K % 128 == 0 else 64}", f"swizzle={int(_swz(M, PW_BM))}")
    if entry in ("adil_pw_join_fwd", "adil_pw_join_bwd"):
        return (entry, f"W={_int(a[-3])}", f"C={_int(a[-2])}")
    if entry == "adil_conv3x3":              # x wp y B H W C N
        B, H, W, C, N = (_int(v) for v in a[3:8])
        bn, tile = (128, 128) if N % 128 == 0 else (64, 256)
        return (entry, f"C={C}", f"N={N}", f"BN={bn}", f"swizzle={int(_swz(B * H * W, tile))}")
    if entry in ("adil_conv3x3_s2_fwd", "adil_conv3x3_s2_bwd"):
        B, H, W, C, N = (_int(v) for v in a[3:8])
        n = N if entry.endswith("fwd") else C
        return (entry, f"C={C}", f"N={N}", f"BN={128 if n % 128 == 0 else 64}", f"swizzle={int(_swz(B * H * W // 4, PW_BM))}")
    if entry == "adil_stem_conv_fwd":        # x x_dtype w mean*3 istd*3 scale shift y B H W
        H, W = _int(a[13]), _int(a[14])
        return (entry, f"dtype={_int(a[1])}", f"whole_tiles={int(H // 2 % 16 == 0 and W // 2 % 16 == 0)}")
    if entry == "adil_stem_conv_bwd":        # gy w istd*3 gx gx_dtype B H W
        H, W = _int(a[8]), _int(a[9])
        return (entry, f"dtype={_int(a[6])}", f"whole_tiles={int(H % 16 == 0 and W % 32 == 0)}")
    if entry in ("adil_affine_act_fwd", "adil_affine_act_bwd"):
        fwd = entry.endswith("fwd")          # fwd: x res scale shift y n C inner relu dtype; bwd: g y scale gx gres n C inner relu dtype
        n, C, inner, relu, dt = (_int(v) for v in a[5:10])
        vec = 4 if dt == 0 else 8
        lay = 0 if inner == 1 and C % vec == 0 else (1 if inner % vec == 0 else 2)
        return (entry, f"dtype={dt}", f"layout={lay}", f"{'res' if fwd else 'gres'}={int(_set(a[1] if fwd else a[4]))}", f"relu={relu}")
    return (entry,)
