/*
 * adil_hip.h — C ABI of libadil_hip.so, the MI355X (gfx950) kernels of the ADiL
 * (Adversarial Dictionary Learning) attack hot path.
 *
 * The upstream reference (flavie-yuan-liu/DL_attack_on_ImageNet) is pure Python on
 * PyTorch: it has no FFI.  Each entry point below replaces a *sequence of torch
 * ops* on the reference's hot path; the reference interface it replaces is cited
 * as file:line.  INTEGRATION.md shows the ctypes stub a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller; the library keeps no
 *     state and allocates nothing persistent; scratch comes in through `ws`.
 *   - `stream` is the caller's hipStream_t (as void*; 0 = default stream).
 *     Kernels are launched asynchronously on it; nothing synchronises.
 *   - return value: 0 on success, otherwise a hipError_t value or one of the
 *     ADIL_E* codes (< 0).  Nothing throws across the boundary.
 *   - the dictionary D is the reference's (C,H,W,K) fp32 tensor, i.e. a
 *     row-major P x K matrix, P = C*H*W, atom index innermost (adil.py:20,25).
 *   - image-shaped streams (x, x_adv, g, z) are row-major B x P, element type
 *     chosen by `dtype` (ADIL_F32 or ADIL_BF16); codes V are fp32 N x K.
 *   - "packed codes": vp is [Bp][Kp] fp32 with Bp = roundup(B,32),
 *     Kp = roundup(K,16), zero padded (see adil_pack_codes).
 */
#ifndef ADIL_HIP_H
#define ADIL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADIL_F32 0
#define ADIL_BF16 1
#define ADIL_U8 2     /* bytes u, value u/255 (correctly rounded fp32): a SOURCE dtype of images only (8-bit image stores) */

#define ADIL_EINVAL (-1)   /* bad argument (null pointer, non-positive size, unsupported K) */
#define ADIL_EWORKSPACE (-2) /* workspace too small */

/* ABI version of this header; bumped on any signature change.  2: frozen-classifier entry points.  3: batch-slot table
 * written by adil_pack_codes and consumed + reset by adil_adamw_l1ball, adil_gather_images, adil_spd_inverse,
 * adil_synth_fp8.  4: device-side stop test arguments of adil_zstep / adil_adamw_l1ball.  5: dyn_scalars of the AdamW
 * entry points incl. adil_zstep (hipGraph replay of the learning step and of the inference iterations).  6: the two
 * helper launches of a gradient pass moved into their neighbours — adil_pack_codes can emit the transposed codes that
 * adil_grad needs (`vpt`) and can take its rows from the grad_v partial sums ("slabs") of a preceding adil_grad;
 * adil_grad can leave the reduction of those slabs to its consumer (`nslabs_out`); adil_adamw_l1ball consumes them.
 * 7: adil_zstep_codes — the z-step of a DDrague iteration also produces the next iteration's codes (as slabs); the
 * persistent fp8 copy of the dictionary (adil_dict_to_fp8, adil_adamw_clamp_fp8, adil_synth_fp8_packed).  8: 8-bit image
 * stores — ADIL_U8 as a source of adil_gather_images, adil_images_to_u8, adil_synth_store.  adil_pw_join_fwd /
 * adil_pw_join_bwd, and after them adil_conv3x3_s2_fwd / adil_conv3x3_s2_bwd, were added under 8: new symbols only, no
 * existing signature changed, and a library without them fails to load by name.  adil_dw3x3_fwd / adil_dw3x3_bwd joined them the
 * same way, and adil_pw8_fwd / adil_pw8_bwd after them, and adil_first3x3_fwd / adil_first3x3_bwd after those, and
 * adil_pool_head_fwd / adil_pool_head_bwd after those, and adil_dense1x1_fwd / adil_dense1x1_bwd after those, and
 * adil_dense3x3_fwd / adil_dense3x3_bwd after those, and their row-pitch forms adil_dense1x1_fwd_ld / adil_dense1x1_bwd_ld /
 * adil_dense3x3_fwd_ld / adil_dense3x3_bwd_ld after those, and adil_dense_transition_fwd / _bwd after those, and adil_bn_pool_head_fwd / adil_bn_pool_head_bwd after those, and
 * adil_attn_max_tokens / adil_attn_fwd / adil_attn_bwd after those: all additive
 * under 8, and so are adil_pw_conv_bwd_tile / adil_pw_route_policy (test and tool entry points: the product calls
 * neither), and adil_pw_conv_fwd_tile after them, and adil_conv3x3_wide / adil_bias_relu_pool2_fwd / _bwd after
 * those, and adil_first3x3_pool_fwd / adil_first3x3_pool_bwd after those.  adil_conv3x3_loop / adil_stem_bwd_variant were two more of that kind, added under 8 and removed again under 8
 * with the kernels they selected: library and binding are built from one tree. */
int adil_abi_version(void);

/* Largest K (atoms) the kernels support. */
int adil_max_atoms(void);

/* Bytes of scratch adil_grad needs for this problem size. */
size_t adil_grad_workspace_bytes(int B, int P, int K);

/* Rows A of the transposed code matrix vpt [A][roundup(B,32)] that adil_grad contracts against (K rounded up to the
 * atom tiling of the kernels: 32, 64 or 128); 0 for an unsupported K. */
int adil_grad_code_rows(int K);

/* Where, inside adil_grad's workspace, the grad_v partial sums live when their reduction is left to the consumer
 * (adil_grad's nslabs_out): `*nslabs_out` slabs of [roundup(B,32)][K] fp32 each, starting this many bytes into ws. */
size_t adil_grad_slab_offset(int B, int P, int K);

/* Gather + pad the batch's code rows:  vp[b][k] = v[index[b]][k] (0 for k>=K, b>=B).
 * Replaces the advanced-indexing `self.v[index, :]` of Attack_dict_model.forward
 * (adil.py:25).  index may be NULL (rows 0..B-1, as adil.py:600 `range(n_img)`).
 * pos (optional, one int32 per row of v, all -1 on entry): pos[index[b]] = b — the batch-slot table that
 * adil_adamw_l1ball consumes; it is what autograd's scatter of the batch gradient into a dense (N,K) grad does.
 * vpt (optional): also the transposed copy vpt[a][b] = vp[b][a], [adil_grad_code_rows(K)][roundup(B,32)] in element
 * type vpt_dtype (ADIL_F32 / ADIL_BF16 = the dtype of the g stream adil_grad will be called with), zero padded:
 * handing it to adil_grad saves that call a launch of its own.
 * slabs / nslabs / slab_rows (nslabs > 0): the rows come from the partial sums a preceding adil_grad left in its
 * workspace instead of from v (v, index ignored; pos must be NULL): row b = sum over the nslabs slabs, in the fixed
 * order of the library's own reduction (bitwise the same values) — the codes `z D_dagger^T` and the code gradient
 * `g D` of a DDrague iteration (adil.py:542, :551) reach the next kernel without a reduction launch in between. */
int adil_pack_codes(const float* v, const int64_t* index, int B, int K, float* vp, int32_t* pos, void* vpt,
                    int vpt_dtype, const float* slabs, int nslabs, int slab_rows, void* stream);

/* Batched image gather, the data step in front of the path (the DataLoader's per-item fetch + torch.stack + .to(device)
 * of adil.py:130-133,168-170 on a dataset that is resident in HBM): dst[b][:] = convert(src[index[b]][:]).
 * src is R x P (src_dtype), dst is B x P (dst_dtype), index may be NULL (rows 0..B-1: a pure cast).  P % 8 == 0. */
int adil_gather_images(const void* src, int src_dtype, const int64_t* index, void* dst, int dst_dtype, int B, int P,
                       void* stream);

/* An 8-bit image store (ADIL_U8): byte u stands for the fp32 value u/255, correctly rounded — bitwise what
 * `uint8 tensor .float().div(255)` (torchvision's ToTensor, DS_ImageNet.py:46) makes of it; bf16 destinations get that
 * value rounded to nearest even, exactly what the fp32 -> bf16 gather makes of it.
 * adil_images_to_u8: dst[i] = rint(255 src[i]) clamped to [0, 255], for n elements of fp32 (src_dtype ADIL_F32; n % 8 == 0,
 * 16-byte aligned src, 8-byte aligned dst) and ADDS to *mismatches (a device counter) the number of elements whose fp32
 * bits differ from those of dst[i]/255, i.e. the elements that are not 8-bit values (the store would change them). */
int adil_images_to_u8(const void* src, int src_dtype, uint8_t* dst, size_t n, unsigned long long* mismatches, void* stream);

/* Perturbation synthesis, fused with the add and the optional clamps:
 *     delta = vp D^T ;  delta = clamp(delta, -delta_clamp, +delta_clamp)   if delta_clamp >= 0
 *     out   = x + delta ;  out = clamp(out, 0, 1)                          if pixel_clamp
 * x may be NULL (out = delta).  Replaces `tensordot(v[index,:], d, ([1],[3]))` + `x + dv`
 * (adil.py:25-26, :543-544, :617), the per-image loop of forward_unsupervised with
 * its +-eps clamp (adil.py:480-484) and the final [0,1] clamp (adil.py:567, :623). */
int adil_synth(const void* x, const float* d, const float* vp, void* out, int B, int P, int K, int dtype,
               float delta_clamp, int pixel_clamp, void* stream);

/* adil_synth with x read straight out of an 8-bit image store: out[b] = store[index[b]]/255 + vp D^T, same clamps, same
 * fusion.  store is R x P bytes (R * P may exceed 4 GB: row offsets are 64-bit), index B int64 rows, out B x P in out_dtype
 * (ADIL_F32 / ADIL_BF16).  fp32 out is bitwise adil_synth on the fp32 gather of the same rows; no gathered copy of the
 * batch is made.  P % 8 == 0, store 4-byte aligned.  There is no fp8 variant. */
int adil_synth_store(const uint8_t* store, const int64_t* index, const float* d, const float* vp, void* out, int B, int P,
                     int K, int out_dtype, float delta_clamp, int pixel_clamp, void* stream);

/* Precision variant of adil_synth for BASELINE.json configs[4] ("fp8 D.V MFMA on CDNA4"; no reference counterpart —
 * the reference contracts in fp32, adil.py:25): both operands of the contraction are converted to fp8 (OCP e4m3) on the
 * fly, the codes scaled by 384 / v_absmax (every |vp| must be <= v_absmax: after update_v the l1 radius eps is such a
 * bound, adil.py:29-31) and the dictionary by 256 (|D| <= 1 after update_d, adil.py:33-35; larger values saturate);
 * products accumulate in fp32 and are scaled back before the add / clamps.  Same arguments and fusion as adil_synth. */
int adil_synth_fp8(const void* x, const float* d, const float* vp, void* out, int B, int P, int K, int dtype,
                   float v_absmax, float delta_clamp, int pixel_clamp, void* stream);

/* The fp8 variant with a PERSISTENT fp8 copy of the dictionary (round 4): adil_synth_fp8 converts the fp32 master on the
 * fly, so it still reads P K 4 bytes of D per launch; here D comes in as the bytes e4m3(256 d) — a quarter of that —
 * produced once by adil_dict_to_fp8 and kept current by adil_adamw_clamp_fp8 (the AdamW + clamp launch of the learning
 * step writes them next to the fp32 master, 1 byte per element on top of its 28).  Same results as adil_synth_fp8, bit
 * for bit (the same encoding of the same values).  P a multiple of 128, K a multiple of 4, 16-byte aligned streams;
 * ADIL_EINVAL otherwise (use adil_synth_fp8).  n must be a multiple of 4 in the two helpers. */
int adil_dict_to_fp8(const float* d, size_t n, void* d_fp8, void* stream);
int adil_adamw_clamp_fp8(float* p, const void* g, int g_dtype, float* m, float* s, size_t n, float decay, float b1,
                         float b2, float eps, float step_size, float bc2_sqrt, float lo, float hi, float* max_abs_delta,
                         const float* dyn_scalars, void* p_fp8, void* stream);
int adil_synth_fp8_packed(const void* x, const void* d_fp8, const float* vp, void* out, int B, int P, int K, int dtype,
                          float v_absmax, float delta_clamp, int pixel_clamp, void* stream);

/* Adjoint of the synthesis in ONE pass over the upstream gradient g = dLoss/d(x+delta):
 *     grad_d  (P x K)  = g^T vp          if grad_d  != NULL   (accumulated into grad_d when accumulate_d)
 *     grad_vb (B x K)  = g D             if grad_vb != NULL
 * Replaces autograd's backward of the tensordot at adil.py:25 (loss.backward(), adil.py:185,
 * :281, :308, :606) and the forward contraction `tensordot(z, d_drg, ([1,2,3],[1,2,3]))`
 * (adil.py:542, :563) when called with g := z and d := D_dagger^T (grad_vb only).
 * vpt (optional): the transposed codes written by adil_pack_codes (element type = dtype); NULL = made here.
 * nslabs_out (optional, HOST int): the caller will consume grad_v through adil_adamw_l1ball / adil_pack_codes, which
 * can sum the per-workgroup partial sums themselves.  When one row chunk covers the batch the reduction launch is
 * skipped, *nslabs_out = number of slabs (at ws + adil_grad_slab_offset, valid until ws is next used) and grad_vb is
 * left untouched; otherwise *nslabs_out = 0 and grad_vb is written as usual (grad_vb must be given either way). */
int adil_grad(const void* g, const float* d, const float* vp, const void* vpt, float* grad_d, float* grad_vb, int B, int P,
              int K, int dtype, int accumulate_d, void* ws, size_t ws_bytes, int* nslabs_out, void* stream);

/* Fused AdamW step + box projection on a flat fp32 parameter (torch.optim.AdamW semantics):
 *     p *= decay ; m += (1-b1)(g-m) ; s = b2 s + (1-b2) g^2 ;
 *     p -= step_size * m / (sqrt(s)/bc2_sqrt + eps) ;  p = clamp(p, lo, hi)
 * decay = 1-lr*wd, step_size = lr/(1-b1^t), bc2_sqrt = sqrt(1-b2^t) are computed by the caller in
 * double, exactly as torch does.  g has element type g_dtype.  If max_abs_delta != NULL,
 * atomically maxes |p_new - p_old| into it (a float the caller zeroed).
 * Replaces optimise.step() + update_d (adil.py:186,188 with :33-35; clamp [-1,1]) and
 * optimise.step() + the z clamp (adil.py:554-555, :559; clamp [-eps,eps]).
 * dyn_scalars (optional, 2 device floats {step_size, bc2_sqrt}): when given they override the by-value arguments, so a
 * launch recorded in a hipGraph can be replayed with the scalars of a later step (the caller refreshes the two floats with
 * a stream-ordered copy before each replay).
 * Arithmetic: fp32, every product, sum, quotient and square root rounded on its own (no contraction, IEEE division,
 * correctly rounded sqrt), in the order p*decay ; m + (1f-b1)*(g-m) ; s*b2 + ((1f-b2)*g)*g ; sqrt(s)/bc2_sqrt + eps ;
 * p - step_size*(m/denom).  The weights are formed as 1.0f - b in fp32 from the fp32 betas: 1.0f - 0.999f =
 * 0.00099998713 and 1.0f - 0.9f = 0.100000024, where torch forms 1 - beta in double (0.001, 0.1): relative differences
 * of 1.3e-5 and 2.4e-7.  This is NOT bitwise torch.optim.AdamW: against torch's fp32 AdamW about 90 % of the bit patterns
 * of p differ after a step (by an ulp or two); against torch's AdamW in float64, three steps on 1e5 N(0,1) elements at
 * lr = 0.01 differ by at most 1.17e-6 in p, inside the bound derived from the two weight differences and the fp32
 * roundings (tests/test_update_reference_cpu.py).  tests/update_reference.py restates the element function operation by
 * operation and tests/test_gpu_update_exact.py requires the kernels' p, m, s and max|delta| to equal it bit for bit.
 * The weights stay as they are: every recorded parity number was measured with them. */
int adil_adamw_clamp(float* p, const void* g, int g_dtype, float* m, float* s, size_t n, float decay, float b1,
                     float b2, float eps, float step_size, float bc2_sqrt, float lo, float hi,
                     float* max_abs_delta, const float* dyn_scalars, void* stream);

/* Fused inference step of forward_supervised_DDrague (adil.py:551-559): the gradient wrt z,
 *     gz = gvp D_dagger   (gvp = packed dLoss/dv [Bp][Kp], dpinv_t = D_dagger^T stored P x K like D),
 * is formed in the MFMA accumulators and consumed on the spot by AdamW(z) + clamp[lo,hi] + max|dz|; it never
 * touches HBM.  z, m, s are fp32 B x P.  Replaces `loss.backward()` through the two tensordots (adil.py:542-543),
 * `optimise.step()`, the clamp (adil.py:555) and the stop test (adil.py:559).
 * Device-side stop test (all three optional, adil.py:559 `if max|z - z_old| < 1e-6: break`): if skip_if_below is
 * given and *skip_if_below < skip_threshold the call changes nothing and sets *max_abs_delta = 0 (so its successor skips
 * as well); otherwise `clear` (a float) is set to 0.  With three floats
 * s[0..2] = {0, 0, +big} and iteration t passing max_abs_delta = &s[t%3], skip_if_below = &s[(t+2)%3], clear =
 * &s[(t+1)%3], every launch after the converged one is a no-op, so the host may read s[t%3] only every few iterations
 * and still end on exactly the iterate the reference breaks at.  dyn_scalars as in adil_adamw_clamp. */
int adil_zstep(float* z, float* m, float* s, const float* dpinv_t, const float* gvp, int B, int P, int K, float decay,
               float b1, float b2, float eps, float step_size, float bc2_sqrt, float lo, float hi, float* max_abs_delta,
               const float* skip_if_below, float skip_threshold, float* clear, const float* dyn_scalars, void* stream);

/* adil_zstep that ALSO leaves the codes of the next iteration, v' = z_new D_dagger^T (adil.py:542, recomputed by the
 * reference from the z that adil.py:554-555 just wrote), as per-workgroup partial sums in `code_slabs`: *nslabs_out slabs
 * of [roundup(B,32)][K] fp32 — the layout adil_grad leaves behind, summed by adil_pack_codes(slabs, nslabs, slab_rows =
 * roundup(B,32)).  The separate contraction launch of a DDrague iteration (adil_grad with g := z: a second pass over z and
 * D_dagger) disappears; the z tile is contracted while it is still in registers, against the D_dagger slice the z-step
 * holds in LDS anyway.  Same arithmetic for z, m, s and the stop test as adil_zstep (bitwise).  A launch skipped by the
 * device-side stop test leaves code_slabs untouched: they keep the codes of the converged z.
 * Shapes: P a multiple of 128 (and < 2^23), K <= 112, 16-byte aligned pointers; adil_zstep_codes_slab_bytes returns the
 * size code_slabs must have, 0 when the shape is not supported (use adil_zstep + adil_grad then). */
size_t adil_zstep_codes_slab_bytes(int B, int P, int K);
int adil_zstep_codes(float* z, float* m, float* s, const float* dpinv_t, const float* gvp, int B, int P, int K, float decay,
                     float b1, float b2, float eps, float step_size, float bc2_sqrt, float lo, float hi, float* max_abs_delta,
                     const float* skip_if_below, float skip_threshold, float* clear, const float* dyn_scalars,
                     float* code_slabs, size_t code_slab_bytes, int* nslabs_out, void* stream);

/* Fused AdamW step on ALL N rows of the code matrix + row-wise l1-ball projection.
 * The gradient is non-zero only for the rows of the current batch: pos[n] = b if row n is
 * batch slot b (gradient row grad_vb[b]), -1 otherwise (zero gradient; the row still
 * moves through momentum and weight decay — reference quirk Q3).  pos may be NULL
 * (row n <-> grad_vb[n], N == B).  With reset_pos every consumed slot is written back to -1, so the table
 * filled by adil_pack_codes is all -1 again for the next batch (no fill / scatter launches in between).
 * grad_vb may be NULL when pos is given and holds no slot (a rank with an empty shard of the batch).
 * radius < 0 skips the projection.
 * Replaces optimise.step() + update_v (adil.py:186-187 with :29-31 and utils.py:21-41),
 * and the same pair in forward_supervised_AdamW (adil.py:609-610, :614); skip_if_below / skip_threshold / clear are the
 * device-side stop test described at adil_zstep (adil.py:614); dyn_scalars as in adil_adamw_clamp.
 * slabs / nslabs / slab_rows (nslabs > 0): the batch gradient is still in the partial sums of the preceding adil_grad
 * (its nslabs_out): gradient row b = sum over the slabs, formed inside this launch; grad_vb is then ignored. */
int adil_adamw_l1ball(float* v, const float* grad_vb, int32_t* pos, int reset_pos, float* m, float* s, int N, int K,
                      float decay, float b1, float b2, float eps, float step_size, float bc2_sqrt, float radius,
                      float* max_abs_delta, const float* skip_if_below, float skip_threshold, float* clear,
                      const float* dyn_scalars, const float* slabs, int nslabs, int slab_rows, void* stream);

/* constraint_dict's third branch (utils.py:55-56: `project_onto_l1_ball(d[:, :, :, ind], eps=1)` per atom): every
 * (channel, atom) row of HW pixels of the (C,H,W,K) dictionary onto the l1 ball of `radius`, in place.  Rows of any
 * length (sort-free threshold search); no caller upstream. */
int adil_atom_l1ball_project(float* d, int C, int HW, int K, float radius, void* stream);

/* Row-wise Euclidean projection onto the l1 ball, in place: project_onto_l1_ball (utils.py:21-41).
 * A row is left untouched when its l1 norm is strictly below the radius (`<`, utils.py:33; the same strict test in
 * adil_atom_l1ball_project and in adil_adamw_l1ball): a row whose norm EQUALS the radius goes through the projection,
 * which finds theta = 0 and returns the same values.  Equal magnitudes are ranked by their index.
 * radius = 0 returns zeros (of either sign) everywhere: no rank passes Duchi's test, rho = 0, theta = 0/0, and
 * fmaxf(|x| - NaN, 0) = 0. */
int adil_l1ball_project(float* x, int N, int K, float radius, void* stream);

/* Row-wise projection onto the l2 ball: x_i *= radius / max(||x_i||_2, radius) (adil.py:626-629). */
int adil_l2ball_project(float* x, int N, int K, float radius, void* stream);

/* ISTA step: v = softshrink(v - step * g, lam)   (g may be NULL: plain softshrink).
 * Replaces Softshrink(step*lambda)(v - step*grad_v) (adil_regularized.py:141-144, :304,
 * :414-416, :570-573; utils.py:159-161). */
int adil_ista_step(float* v, const float* g, size_t n, float step, float lam, void* stream);

/* Per-atom Frobenius norms of D: norms[k] = ||D[:,k]||_2   (utils.py:48). ws: adil_atom_workspace_bytes. */
size_t adil_atom_workspace_bytes(int P, int K);
int adil_atom_norms(const float* d, int P, int K, float* norms, void* ws, size_t ws_bytes, void* stream);

/* Per-atom scaling: d[:,k] /= (sphere ? norms[k] : max(norms[k], 1))   (utils.py:49-54). */
int adil_atom_scale(float* d, int P, int K, const float* norms, int sphere, void* stream);

/* Gram matrix  gram (K x K) = D^T D   (adil.py:523), fp32-grade on the matrix pipe (split bf16 MFMAs), bitwise
 * reproducible.  ws: adil_gram_workspace_bytes(P, K) bytes of device scratch (per-workgroup partial sums). */
size_t adil_gram_workspace_bytes(int P, int K);
int adil_gram(const float* d, int P, int K, float* gram, void* ws, size_t ws_bytes, void* stream);

/* out (K x K) = a^-1 for a symmetric positive definite K x K matrix (the Gram matrix; `dtd.inverse()`, adil.py:524).
 * One workgroup, fp64 Gauss-Jordan in LDS; no host round trip. */
int adil_spd_inverse(const float* a, int K, float* out, void* stream);

/* out (P x K) = D M^T  with M (K x K):  D_dagger^T = D (DtD^-1)^T   (adil.py:525, stored P x K); fp32-grade on the
 * matrix pipe (split bf16 MFMAs). */
int adil_dict_rightmul(const float* d, const float* mat, int P, int K, float* out, void* stream);

/* Per-image evaluation sums (performance.py:249-266): sq_err[b] = sum_p (adv-x)^2, sq_norm[b] = sum_p x^2. */
int adil_image_metrics(const void* adv, const void* x, int B, int P, int dtype, float* sq_err, float* sq_norm,
                       void* stream);

/* Precondition of the ReLU masks of adil_pw_conv_bwd and adil_pw_join_bwd: the tensor a mask [y > 0] is taken from (y, h1,
 * out) must not hold -0.0.  Those two kernels test the sign of the 16-bit pattern, so -0.0 would count as positive.
 * adil_pw_conv_fwd and adil_pw_join_fwd clip with an integer max on the bf16 pattern and write +0 also for a -0.0
 * pre-activation (a negative scale times a zero accumulator plus a -0.0 shift: a row of
 * tests/test_gpu_classifier_routes.py), so a y they produced qualifies.  adil_affine_act_bwd compares values (y > 0.0f) in
 * both dtypes and has no such precondition.
 *
 * Frozen-classifier epilogues (NOT part of the ADiL maths; no reference counterpart — they replace the separate
 * BatchNorm(eval) / add / ReLU kernels PyTorch launches around each convolution of the frozen network, e.g. the
 * torchvision ResNet blocks the reference builds at demo_dL_attack.py:41-59):
 *     y = act( x * scale[c] + shift[c] (+ res) ),  act = ReLU if relu else identity
 *     gx = mask * g * scale[c],  gres = mask * g  (mask = y > 0 if relu else 1)     [input gradient only: frozen net]
 * channel of flat element i is (i / inner) % C  (inner = 1 for channels_last storage, H*W for NCHW); n % 8 == 0. */
int adil_affine_act_fwd(const void* x, const void* res, const float* scale, const float* shift, void* y, size_t n, int C,
                        int inner, int relu, int dtype, void* stream);
int adil_affine_act_bwd(const void* g, const void* y, const float* scale, void* gx, void* gres, size_t n, int C,
                        int inner, int relu, int dtype, void* stream);

/* Frozen-classifier stem, the stage on either side of the hot path for the torchvision ResNets the reference attacks
 * (demo_dL_attack.py:41-59; NOT part of the ADiL maths): Normalize -> conv 7x7/2 (3->64) -> BatchNorm(eval) -> ReLU ->
 * maxpool 3x3/2, forward and input gradient, on the attack's own layouts (x_adv / dLoss/dx_adv are B x 3 x H x W in the
 * stream dtype; activations are NHWC bf16).  H and W even.  Weights are pre-packed bf16:
 *     w_fwd [64][7][8][4]  = w[co][ci][kh][kw] at [co][kh][kw][ci], zero for kw = 7 / ci = 3
 *     w_bwd [4][49][64]    = w[co][ci][kh][kw] at [ci][kh*7+kw][co], zero for ci = 3
 *   adil_stem_conv_fwd : y1 = relu((conv((x - mean) * inv_std)) * scale[co] + shift[co]),  y1 is B x H/2 x W/2 x 64
 *   adil_maxpool_fwd   : p = maxpool3x3/2/pad1(y) (B x OH x OW x C -> B x PH x PW x C, PH = (OH-1)/2+1), idx = position
 *                        kh*3+kw of the first maximum (torch.nn.functional.max_pool2d's rule); C % 8 == 0
 *   adil_stem_pool_bwd : gy = route(g; idx) * [p > 0] * scale[c]   (maxpool + ReLU + BatchNorm backward, B x OH x OW x C)
 *   adil_stem_conv_bwd : gx = inv_std[ci] * conv7x7/2 input gradient of gy   (B x 3 x H x W, gx_dtype)
 * The two convolutions take 1 <= B <= 65535 (the forward's image index is a grid dimension).  ADIL_EINVAL, before any
 * launch, for a NULL pointer, a non-positive size, odd H or W, B > 65535, a dtype code outside the two, (pooling)
 * C % 8 != 0, or a shape beyond the backward kernels' grids, which no image tensor comes near:
 *   adil_stem_pool_bwd : B * PH > 2^31 - 1 (a row of 2 x 2 pixel quads per workgroup row), or
 *                        ceil(PW * (C / 8) / 256) > 65535 (the workgroups along such a row)
 *   adil_stem_conv_bwd : more than 2^31 - 1 tiles of 32 x 16 input pixels, B * ceil(W / 32) * ceil(H / 16)
 * adil_stem_conv_bwd computes the four input-pixel parity classes (h & 1, w & 1) in one MFMA per (g_y1 shift, channel
 * half).  For every finite gy that is bit for bit the sum over each class's own taps (kh, then kw ascending).  A
 * non-finite gy value meets the zero weights of the classes that have no tap at its shift: 0 * inf = NaN then also
 * reaches input pixels of another parity whose own taps do not read that value.
 * Arithmetic of the pooling pair (restated in tests/stem_pool_reference.py, which the kernels must equal bit for bit):
 *   adil_maxpool_fwd   : the window of (ph, pw) is the taps (kh, kw), scanned in the order kh*3+kw, whose pixel
 *                        (2ph-1+kh, 2pw-1+kw) lies inside the grid; padding taps are ABSENT, not zeros (a window of negative
 *                        values has a negative maximum).  p is the first maximum under > (+0 and -0 compare equal: the
 *                        earlier one stays, with its sign); a NaN always replaces the running value, so the LAST NaN of a
 *                        window wins.  idx is that tap's kh*3+kw.  p is a selection: it carries the input's bit pattern
 *                        (a NaN stays a NaN).
 *   adil_stem_pool_bwd : per element of gy, the fp32 sum, in ascending (ph, pw) order, of the at most four g whose window
 *                        contains the pixel, whose idx names it and whose p > 0 BY VALUE (-0, negatives and NaN fail), then
 *                        ONE fp32 product with scale[c] and ONE rounding to bf16, to nearest even.  Every element of gy is
 *                        written (an element no window routes to is a zero); no sign of zero is promised. */
int adil_stem_conv_fwd(const void* x, int x_dtype, const void* w_fwd, float mean0, float mean1, float mean2, float inv_std0,
                       float inv_std1, float inv_std2, const float* scale, const float* shift, void* y, int B, int H, int W,
                       void* stream);
int adil_maxpool_fwd(const void* y, void* p, uint8_t* idx, int B, int OH, int OW, int C, void* stream);
int adil_stem_pool_bwd(const void* g, const uint8_t* idx, const void* p, const float* scale, void* gy, int B, int OH, int OW,
                       int C, void* stream);
int adil_stem_conv_bwd(const void* gy, const void* w_bwd, float inv_std0, float inv_std1, float inv_std2, void* gx,
                       int gx_dtype, int B, int H, int W, void* stream);

/* Pointwise (1x1) convolution of the frozen network on channels_last storage, with the eval-BatchNorm / residual /
 * ReLU epilogue applied to the accumulators (bf16 in/out, fp32 accumulate):
 *     y[M][N] = act( (x'[M][K] . w[N][K]^T) * scale[n] + shift[n] (+ res[M][N]) ),  M = output pixels, K = Cin, N = Cout
 * K % 64 == 0, N % 64 == 0; res may be NULL; relu = 0/1.
 * Stride 2 (the ResNet downsample convolutions): sub_w = OW > 0, sub_hw = OH*OW: output pixel (n,oh,ow) reads input
 * pixel (n,2oh,2ow) of the B x 2OH x 2OW x K tensor x points to (gathered, nothing copied); sub_w = 0: stride 1.
 * Optional prologue (pscale, pshift both non-NULL, K <= 512): x is the RAW output of the previous convolution and
 * x' = relu(x * pscale[k] + pshift[k]) is formed on the operand path (its BatchNorm + ReLU never makes an HBM pass);
 * otherwise x' = x. */
int adil_pw_conv_fwd(const void* x, const void* w, const float* scale, const float* shift, const void* res, void* y, int M,
                     int K, int N, int relu, const float* pscale, const float* pshift, int sub_w, int sub_hw, void* stream);
/* Input gradient of adil_pw_conv_fwd (of the stride-1 form; a stride-2 layer calls it with M = its output pixels and
 * gets the gradient on its own stride-2 grid).  v = g (+ g2) (+ up2(g3)), mask = [y > 0] if relu else 1:
 *     gres[M][N] = v * mask (optional),   gx[M][K] = (v * mask * scale[n]) . w,   weight given transposed, wt[K][N].
 * g2 (optional): the second gradient meeting at a residual join.  g3 (optional, with sub_w = OW, sub_hw = OH*OW,
 * M = B*4*OH*OW): a gradient living on the stride-2 grid, [M/4][N]; pixel (n,h,w) receives g3[(n,h/2,w/2)] for even
 * h and w (the zero-upsampled tensor is never materialised).  N % 64 == 0, K % 64 == 0, N <= 2048.
 * With the forward's prologue (xin = the raw x, pscale, pshift) the result is the gradient wrt xin:
 *     gx *= [xin * pscale + pshift > 0] * pscale.
 * This epilogue reads pscale / pshift from global memory, so unlike the forward's prologue it has no K <= 512 limit.
 * y must not hold -0.0 (see "Precondition of the ReLU masks" above). */
int adil_pw_conv_bwd(const void* g, const void* g2, const void* y, const float* scale, const void* wt, void* gx, void* gres,
                     int M, int K, int N, int relu, const void* xin, const float* pscale, const float* pshift, const void* g3,
                     int sub_w, int sub_hw, void* stream);
/* adil_pw_conv_bwd picks the output-channel tile of its workgroups (64, 128, or the wide 256 / 512 of the 8-wave form)
 * from K, N and M; every tile gives the same bits, so the choice is one of speed only.  For tests and tools:
 * adil_pw_conv_bwd_tile is the same call at the forced tile `bo`; bo outside {64, 128, 256, 512}, K % bo != 0, or
 * bo >= 256 with g3 set (the wide tiles have no g3 form): ADIL_EINVAL before any launch, outputs untouched.
 * adil_pw_route_policy sets how adil_pw_conv_bwd chooses (a host-side int read at launch; 0 = the measured table, the
 * default; 1 = the narrow tiles 128 / 64 everywhere; 2 = the widest tile dividing K wherever one covers the call) and
 * returns the previous value; any other argument changes nothing and only returns the current value. */
int adil_pw_conv_bwd_tile(const void* g, const void* g2, const void* y, const float* scale, const void* wt, void* gx,
                          void* gres, int M, int K, int N, int relu, const void* xin, const float* pscale,
                          const float* pshift, const void* g3, int sub_w, int sub_hw, void* stream, int bo);
int adil_pw_route_policy(int policy);
/* adil_pw_conv_fwd picks its output-channel tile the same way (64, 128, or the wide 256 / 512 of an 8-wave form that
 * stages the x operand once per workgroup) from K, N and M, under the same adil_pw_route_policy (2 = the widest tile
 * dividing N); every tile gives the same bits.  adil_pw_conv_fwd_tile is the same call at the forced tile `bn`, for tests
 * and tools: bn outside {64, 128, 256, 512} or N % bn != 0: ADIL_EINVAL before any launch, y untouched. */
int adil_pw_conv_fwd_tile(const void* x, const void* w, const float* scale, const float* shift, const void* res, void* y,
                          int M, int K, int N, int relu, const float* pscale, const float* pshift, int sub_w, int sub_hw,
                          void* stream, int bn);

/* Residual join of two consecutive bottlenecks of one stage (conv3 of block i-1 and conv1 of block i) as ONE kernel;
 * the C-channel tensor between the two GEMMs is kept on chip.  W = width in {64, 128}, C = 4 W, M = pixels; bf16
 * channels_last storage; w3 [C][W], w1 [W][C].  The results are bitwise those of
 *     adil_pw_conv_fwd(h2raw, w3, scale3, shift3, res, out, M, W, C, 1, pscale2, pshift2, 0, 0)      (conv3, block i-1)
 *     adil_pw_conv_fwd(out, w1, scale1, shift1, NULL, h1, M, C, W, 1, NULL, NULL, 0, 0)              (conv1, block i)
 * Any other W: ADIL_EINVAL (the caller keeps the two calls). */
int adil_pw_join_fwd(const void* h2raw, const float* pscale2, const float* pshift2, const void* w3, const float* scale3,
                     const float* shift3, const void* res, void* out, const void* w1, const float* scale1,
                     const float* shift1, void* h1, int M, int W, int C, void* stream);
/* Input gradient of adil_pw_join_fwd, bitwise that of (t [M][C] is never written)
 *     adil_pw_conv_bwd(g_h1, NULL, h1, scale1, wt1, t, NULL, M, C, W, 1, NULL, NULL, NULL, NULL, 0, 0)
 *     adil_pw_conv_bwd(t, g_out, out, scale3, wt3, gx, gres, M, W, C, 1, h2raw, pscale2, pshift2, NULL, 0, 0)
 * with the transposed weights wt1 [C][W] (of w1) and wt3 [W][C] (of w3); gres = gradient of res, gx = of h2raw.
 * h1 and out must not hold -0.0 (see "Precondition of the ReLU masks" above). */
int adil_pw_join_bwd(const void* g_h1, const void* h1, const float* scale1, const void* wt1, const void* g_out,
                     const void* out, const float* scale3, void* gres, const void* wt3, const void* h2raw,
                     const float* pscale2, const float* pshift2, void* gx, int M, int W, int C, void* stream);

/* 3x3 / stride 1 / pad 1 convolution of the frozen network on channels_last storage, raw bf16 output (its BatchNorm +
 * ReLU run in the next pointwise kernel's prologue):  y[B][H][W][N] = conv3x3(x[B][H][W][C]; wp), weights packed
 * wp[N][9][C] = w[n][c][kh][kw] at [n][kh*3+kw][c].  The input gradient is the same call on wp' [C][9][N] =
 * w[n][c][2-kh][2-kw] at [c][kh*3+kw][n].  C % 64 == 0, N % 64 == 0, W <= 63, and the weight pack 9 * C * N below 2^31
 * elements (the kernel indexes it with 32 bits); anything else: ADIL_EINVAL before any launch. */
int adil_conv3x3(const void* x, const void* wp, void* y, int B, int H, int W, int C, int N, void* stream);

/* 3x3 / stride 2 / pad 1 convolution of the frozen network on channels_last storage (conv2 of the first bottleneck of
 * stages 2-4, conv1 of the same BasicBlocks), raw bf16 output, bf16 MFMA with fp32 accumulation, one rounding.
 * H, W are the INPUT grid in both calls (even), the stride-2 grid is OH x OW = H/2 x W/2:
 *   adil_conv3x3_s2_fwd : y[B][OH][OW][N] = sum x[b][2oh-1+kh][2ow-1+kw][c] * w[n][c][kh][kw],  x is [B][H][W][C],
 *                         weights packed as for adil_conv3x3: wp[N][9][C] = w[n][c][kh][kw] at [n][kh*3+kw][c]
 *   adil_conv3x3_s2_bwd : gx[B][H][W][C] = sum g[b][(h+1-kh)/2][(w+1-kw)/2][n] * w[n][c][kh][kw] over the taps whose
 *                         quotients are integers and in range (1 / 2 / 2 / 4 taps by the parity of (h, w); g is never
 *                         zero-upsampled), g is [B][OH][OW][N], weights wp_bwd[C][9][N] = w[n][c][kh][kw] at
 *                         [c][kh*3+kw][n] (taps NOT flipped, channels swapped).  Every element of gx is written.
 * C % 64 == 0, N % 64 == 0 (C != N allowed), H and W even, W <= ADIL_CONV3X3_S2_MAX_W (the width limit of adil_conv3x3:
 * image sizes whose stride-1 3x3 layers run here), 9 * C * N below 2^31 (as adil_conv3x3); anything else: ADIL_EINVAL
 * before any launch, outputs untouched.
 * No atomics: bitwise reproducible. */
#define ADIL_CONV3X3_S2_MAX_W 63
int adil_conv3x3_s2_fwd(const void* x, const void* wp, void* y, int B, int H, int W, int C, int N, void* stream);
int adil_conv3x3_s2_bwd(const void* g, const void* wp_bwd, void* gx, int B, int H, int W, int C, int N, void* stream);

/* Depthwise 3x3 / pad 1 / stride 1 or 2 convolution (groups == channels: the 17 such layers of MobileNetV2) of the frozen
 * network on channels_last storage, with the layer's eval-BatchNorm folded into the weights and its ReLU6 applied in the
 * same pass: bf16 in / out, fp32 arithmetic, ONE rounding to bf16 (nearest even).  H, W are the INPUT grid in both calls,
 * any H, W >= 1 (odd sizes included); the output grid is OH x OW = (H-1)/stride + 1 x (W-1)/stride + 1.
 *   w    [9][C] fp32 = w[c][kh][kw] * scale[c] at [kh*3+kw][c]   (scale = gamma / sqrt(var + eps), derived in fp64)
 *   bias [C] fp32    = beta - mean * scale; may be NULL (no bias)
 *   adil_dw3x3_fwd : y[b][oh][ow][c] = act( sum x[b][s oh-1+kh][s ow-1+kw][c] * w[kh*3+kw][c] + bias[c] ),  x is [B][H][W][C],
 *                    act = min(max(., 0), 6) if relu6 else the identity
 *   adil_dw3x3_bwd : gx[b][h][w][c] = sum (g m)[b][(h+1-kh)/s][(w+1-kw)/s][c] * w[kh*3+kw][c] over the taps whose quotients
 *                    are integers and in range (g is never zero-upsampled), g and y are [B][OH][OW][C];
 *                    m = [0 < y < 6] taken from the stored bf16 y by comparing VALUES (so -0.0 in y is simply a zero: no
 *                    precondition, unlike adil_pw_conv_bwd); relu6 == 0: m = 1 and y may be NULL.
 *                    Every element of gx is written.  Input gradient only: the network is frozen.
 * C % 8 == 0 (16-byte lanes), 16-byte aligned pointers; anything else, a stride outside {1, 2}, a non-positive size or a NULL
 * mandatory pointer: ADIL_EINVAL before any launch, outputs untouched.  Element offsets are 64-bit (B H W C may pass 2^31).
 * No atomics: bitwise reproducible. */
int adil_dw3x3_fwd(const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int C, int stride,
                   int relu6, void* stream);
int adil_dw3x3_bwd(const void* g, const void* y, const float* w, void* gx, int B, int H, int W, int C, int stride,
                   int relu6, void* stream);

/* Pointwise (1x1, stride 1) convolution of the frozen network for channel counts that are multiples of 8 (the 34 such
 * layers of MobileNetV2: 16 / 24 / 32 / 96 / 144 / 160 / 192 / 320 / 384 / 576 / 960 / 1280 channels) on channels_last
 * storage, i.e. a row-major GEMM over M = B H W pixels, with the layer's eval-BatchNorm, the residual add and the ReLU6
 * clamp applied on the accumulators: bf16 in / out, bf16 MFMA with fp32 accumulation, fp32 epilogue, ONE rounding to bf16
 * (nearest even).
 *   scale, shift [N] fp32 : scale = gamma / sqrt(var + eps), shift = beta - mean * scale (derived in fp64)
 *   adil_pw8_fwd : y[M][N] = act( (x[M][K] . w[N][K]^T) * scale[n] + shift[n] (+ res[M][N]) ),
 *                  act 0 = the identity (the linear bottleneck), act 1 = min(max(., 0), 6) before the rounding; every
 *                  pre-activation <= 0 is written as +0, never -0.0.  res may be NULL and is allowed only with act 0.
 *   adil_pw8_bwd : gz = bf16(g * scale[n]) (one fp32 product, one rounding), with act 1 masked by [0 < y < 6];
 *                  gx[M][K] = gz . wt^T with wt[K][N] the TRANSPOSED weight (the reduction index is contiguous, as in
 *                  adil_pw_conv_bwd).  The mask is taken from the stored bf16 y by comparing VALUES (-0.0 in y is a zero:
 *                  no precondition); act 0: y may be NULL.  There is no gradient output for res: it is g itself.
 *                  Every element of gx is written.  Input gradient only: the network is frozen.
 * K % 8 == 0, N % 8 == 0, 8 <= K, N <= 2048 (no multiple of 16, 32 or 64 is needed), any M >= 1, 16-byte aligned
 * pointers; anything else, a NULL mandatory pointer, res with act 1 or act outside {0, 1}: ADIL_EINVAL before any launch,
 * outputs untouched.  No load or store leaves the M x K, N x K, M x N extents: the K tail and the N tail are clipped and
 * zero-filled.  Element offsets are 64-bit (M N may pass 2^31).  One launch on `stream`, no synchronisation, no
 * allocation.  No atomics: bitwise reproducible. */
int adil_pw8_fwd(const void* x, const void* w, const float* scale, const float* shift, const void* res, void* y, int M,
                 int K, int N, int act, void* stream);
int adil_pw8_bwd(const void* g, const void* y, const float* scale, const void* wt, void* gx, int M, int K, int N, int act,
                 void* stream);

/* First convolution of the frozen MobileNetV2 (features[0]: 3 -> 32, 3x3, stride 2, pad 1, no bias) with the Normalize in
 * front of it and its eval-BatchNorm + ReLU6 behind it, forward and input gradient, on the attack's own layouts: x_adv /
 * dLoss/dx_adv are [B][3][H][W] NCHW in the stream dtype (ADIL_F32 / ADIL_BF16, the codes of adil_stem_conv_fwd), the
 * activation side is [B][OH][OW][32] channels_last bf16.  H, W are the INPUT grid in both calls, any H, W >= 1 (odd sizes
 * included); OH x OW = (H-1)/2 + 1 x (W-1)/2 + 1.  bf16 MFMA with fp32 accumulation.  Weights are pre-packed bf16:
 *     w_fwd [32][3][4][4] = w[n][c][kh][kw] at [n][kh][kw][c], zero for kw = 3 / c = 3 (K = 27 padded to 3 x 16)
 *     w_bwd [3][9][32]    = w[n][c][kh][kw] at [c][kh*3+kw][n] (taps NOT flipped, channels swapped, as adil_conv3x3_s2_bwd)
 *   scale, shift [32] fp32 : scale = gamma / sqrt(var + eps), shift = beta - mean * scale (derived in fp64)
 *   adil_first3x3_fwd : x' = bf16( f32( f32(x - mean[c]) * inv_std[c] ) ): the subtraction and the product each rounded to
 *                       fp32, then nearest even to bf16; padding taps are zeros of x', not of x;
 *                       acc = sum x'[b][c][2oh-1+kh][2ow-1+kw] * w[n][c][kh][kw] in fp32 (any order);
 *                       y = bf16( act( acc * scale[n] + shift[n] ) ), act = min(max(., 0), 6) if relu6 else the identity;
 *                       every pre-activation <= 0 (relu6) and every zero (relu6 == 0) is written as +0, never -0.0.
 *   adil_first3x3_bwd : gz = bf16(g * scale[n]) (one fp32 product, one rounding), with relu6 masked by [0 < y < 6] taken
 *                       from the stored bf16 y by comparing VALUES (-0.0 in y is a zero); relu6 == 0: y may be NULL;
 *                       gx[b][c][h][w] = round( inv_std[c] * sum gz[b][(h+1-kh)/2][(w+1-kw)/2][n] * w[n][c][kh][kw] ) over the
 *                       taps whose quotients are integers and in range (1 / 2 / 2 / 4 taps by the parity of (h, w); g is
 *                       never zero-upsampled): fp32 sum in any order, ONE fp32 multiply by inv_std, one rounding when gx is
 *                       bf16.  Every element of gx is written.  Input gradient only: the network is frozen.
 * 16-byte aligned y, g, w_fwd, w_bwd; x and gx aligned to their element size.  A NULL mandatory pointer, a non-positive
 * size, B > 65535 (the image index is a grid dimension), a dtype code outside the two, relu6 outside {0, 1} or a misaligned
 * pointer: ADIL_EINVAL before any launch, outputs untouched.  No load leaves the extents of x, g or y: border taps are
 * predicated, never clamped reads.  Element offsets are 64-bit (B OH OW 32 passes 2^31 at B ~ 5350 for 224 x 224).  One
 * launch on `stream`, no synchronisation, no allocation.  No atomics: bitwise reproducible. */
int adil_first3x3_fwd(const void* x, int x_dtype, const void* w_fwd, float mean0, float mean1, float mean2, float inv_std0,
                      float inv_std1, float inv_std2, const float* scale, const float* shift, void* y, int B, int H, int W,
                      int relu6, void* stream);
int adil_first3x3_bwd(const void* g, const void* y, const float* scale, const void* w_bwd, float inv_std0, float inv_std1,
                      float inv_std2, void* gx, int gx_dtype, int B, int H, int W, int relu6, void* stream);

/* Global average pooling + the last linear layer of the frozen classifier with fp32 logits, forward and input gradient, on
 * the channels_last bf16 activation itself (the head of MobileNetV2: C = 1280, 7 x 7; the ResNet widths 512 and 2048 are
 * covered too).  Only x and gx are bf16; weights, pooled features, logits and their gradients are fp32.
 *     x, gx           [B][HW][C] bf16 : the channels_last storage of a (B, C, H, W) activation, HW = H W
 *     w               [N][C] fp32     : the Linear's own layout (read by the backward, contiguous in c)
 *     wt              [C][N] fp32     : its transpose (read by the forward, contiguous in n)
 *     bias            [N] fp32
 *     g, logits       [B][N] fp32
 *     pooled, gpooled [B][C] fp32     : caller-provided OUTPUTS with defined values, not scratch
 *   inv_hw = 1.0f / (float)HW, formed on the host.
 *   adil_pool_head_fwd : S[b][c] = sum_hw x[b][hw][c] in fp32 (any order); pooled[b][c] = f32(S * inv_hw): ONE fp32 multiply;
 *                        logits[b][n] = bias[n] + sum_c pooled[b][c] * w[n][c]: fp32 products and sums in any order, the
 *                        bias at any position of the sum; the factors are the stored fp32 values themselves (no bf16
 *                        rounding of pooled or w, no split).
 *   adil_pool_head_bwd : gpooled[b][c] = sum_n g[b][n] * w[n][c] in fp32 (any order);
 *                        gx[b][hw][c] = bf16( f32(gpooled[b][c] * inv_hw) ), nearest even, the same value for every hw.
 *                        Every element of gx is written.  Input gradient only: the network is frozen.
 * C % 8 == 0, 8 <= C <= 2048, 1 <= HW <= 65536, 1 <= B <= 65535 (the image index is a grid dimension), 1 <= N <= 65535:
 * every N is correct, multiples of 4 take 16-byte loads and stores, the others element-wise ones.  x, gx, w, wt, g, logits,
 * pooled, gpooled 16-byte aligned, bias 4-byte aligned.  A NULL pointer, a size outside these ranges or a misaligned
 * pointer: ADIL_EINVAL before any launch, outputs untouched.  No load leaves the extents of an operand: the tails in B, C,
 * HW and N are predicated, never clamped or over-read.  Element offsets are 64-bit (B HW C may pass 2^31).  Two launches
 * per call on `stream` (a stream pass over x / gx and a small GEMM), no synchronisation, no allocation.  No atomics: bitwise
 * reproducible. */
int adil_pool_head_fwd(const void* x, const float* wt, const float* bias, float* pooled, float* logits, int B, int HW,
                       int C, int N, void* stream);
int adil_pool_head_bwd(const float* g, const float* w, float* gpooled, void* gx, int B, int HW, int C, int N, void* stream);

/* The same head behind an eval-BatchNorm + ReLU (DenseNet-121: norm5, ReLU, global pooling, classifier): the activation in
 * front of the BatchNorm is read once for fp32 pooled features and fp32 logits, and read once more for the input gradient.
 * Operands as above, and
 *     pscale, pshift  [C] fp32 : the BatchNorm (scale = gamma / sqrt(var + eps), shift = beta - mean * scale)
 *   pre[b][hw][c] = fadd_rn(fmul_rn(f32(x[b][hw][c]), pscale[c]), pshift[c]): the prologue of adil_dense1x1_fwd, two fp32
 *   roundings and no contraction; p = pre > 0 ? pre : +0 (-0.0 and NaN give +0).  p is never rounded to bf16.
 *   adil_bn_pool_head_fwd : S[b][c] = sum_hw p in fp32, in adil_pool_head_fwd's order (the pixels hw = r, r + 8, ... in
 *                           ascending order for r = 0 .. 7, then the eight partial sums r = 0 .. 7 in ascending order);
 *                           pooled = f32(S * inv_hw); logits as adil_pool_head_fwd.
 *   adil_bn_pool_head_bwd : gpooled as adil_pool_head_bwd; v[b][c] = f32(f32(gpooled[b][c] * inv_hw) * pscale[c]), two fp32
 *                           products in this order; gx[b][hw][c] = bf16_rne(v[b][c]) where pre[b][hw][c] > 0, else +0; pre is
 *                           recomputed from x.  Every element of gx is written; gx must not overlap x.
 * Limits, alignment (pscale and pshift 16-byte aligned too), refusals, predication, 64-bit offsets, launches and
 * reproducibility as adil_pool_head_*. */
int adil_bn_pool_head_fwd(const void* x, const float* pscale, const float* pshift, const float* wt, const float* bias,
                          float* pooled, float* logits, int B, int HW, int C, int N, void* stream);
int adil_bn_pool_head_bwd(const float* g, const float* w, const void* x, const float* pscale, const float* pshift,
                          float* gpooled, void* gx, int B, int HW, int C, int N, void* stream);

/* Pre-activated pointwise (1x1, stride 1) convolution of the frozen DenseNet-121: the eval-BatchNorm + ReLU IN FRONT of the
 * convolution (on the concatenated input of a dense layer or a transition, K = 64 .. 1024 in steps of 32) is applied on the
 * way into the GEMM, the eval-BatchNorm + ReLU behind it on the accumulators; forward and input gradient, one kernel each
 * way.  channels_last bf16 storage, M = B H W pixels:
 *     x, xin, gx     [M][K] bf16
 *     w              [N][K] bf16, wt [K][N] bf16 its transpose
 *     pscale, pshift [K] fp32 : the BatchNorm in front (scale = gamma / sqrt(var + eps), shift = beta - mean * scale)
 *     scale, shift   [N] fp32 : the BatchNorm behind
 *     y, g           [M][N] bf16
 *   Prologue : pre[m][k] = fadd_rn(fmul_rn(f32(x[m][k]), pscale[k]), pshift[k]): the product and the sum are each rounded
 *              to fp32, no contraction, so an fp32 restatement reproduces the branch and the bits;
 *              a = bf16_rne(max(pre, 0)); every pre <= 0 gives +0.
 *   adil_dense1x1_fwd : acc = sum_k a[m][k] * w[n][k], bf16 MFMA with fp32 accumulation in any order;
 *                       y = bf16_rne(act(acc * scale[n] + shift[n])); act 1 = ReLU, NOT ReLU6: max(., 0), non-positive
 *                       values written as +0; act 0 = the identity (a transition calls it with scale = 1, shift = 0; there
 *                       is no NULL special case).
 *   adil_dense1x1_bwd : gz = bf16_rne(g * scale[n]): one fp32 product, one rounding; with act 1, gz is masked by [y > 0],
 *                       taken from the stored bf16 y by comparing VALUES (-0.0 is a zero; there is no precondition);
 *                       t = sum_n gz[m][n] * wt[k][n] in fp32; gx[m][k] = bf16_rne(t * pscale[k]) where pre[m][k] > 0,
 *                       else +0; pre is recomputed from xin by the forward's two operations, so the mask is the forward's
 *                       branch.  Every element of gx is written.  Input gradient only: the network is frozen.  With act 0,
 *                       y may be NULL.
 * Limits as adil_pw8_*: K % 8 == 0, N % 8 == 0, 8 <= K, N <= 2048, any M >= 1, 16-byte aligned bf16 pointers, 4-byte aligned
 * tables.  A NULL mandatory pointer, act outside {0, 1}, a size outside the limits or a misaligned pointer: ADIL_EINVAL
 * before any launch, outputs untouched.  No load or store leaves an operand's extent, the [K] / [N] tables included: tails
 * in M, K and N are clipped and zero-filled on BOTH MFMA operands.  Element offsets are 64-bit.  One launch per call on
 * `stream`, no allocation, no synchronisation.  No atomics: bitwise reproducible. */
int adil_dense1x1_fwd(const void* x, const float* pscale, const float* pshift, const void* w, const float* scale,
                      const float* shift, void* y, int M, int K, int N, int act, void* stream);
int adil_dense1x1_bwd(const void* g, const void* y, const float* scale, const void* wt, const void* xin, const float* pscale,
                      const float* pshift, void* gx, int M, int K, int N, int act, void* stream);
/* The same two calls on operands that are column slices of wider channels_last buffers (the feature buffer
 * [B][H][W][Ctot] of a dense block and its gradient buffer).  Every ld* is a row pitch in ELEMENTS: row m of a strided
 * operand starts at base + m * ld and only its first `width` elements belong to the operand (width = K for x, xin, gx;
 * N for y, g).  Columns at or behind the width are never read (the zero-filled 16-byte chunk past the reduction extent
 * is read at an address inside the width) and, on the output, never written: in the gradient buffer they hold the live
 * gradients of other slices.  w, wt and the tables stay dense.  Everything else is the plain call, which IS this one at
 * ld = width and accumulate = 0 (same launcher, same bits).
 *   accumulate (adil_dense1x1_bwd_ld): 0 = gx is written as by adil_dense1x1_bwd.  1 = gx[m][k] = bf16_rne(f32(gx_old[m][k])
 *     + v) with v the fp32 value t * pscale[k] where pre[m][k] > 0 and +0.0f elsewhere: ONE fp32 add (not contracted with
 *     the product) and ONE rounding to bf16; v itself is never rounded to bf16.  An old -0.0 under a masked element becomes
 *     +0.  Every element of the K-wide prefix of a row is read once and written once, by the wave that owns the pixel
 *     row; no atomics, bitwise reproducible.
 * Limits: those of the plain calls, and every ld >= its operand's width, every ld % 8 == 0 (16-byte rows), accumulate in
 * {0, 1} (ldy is checked also where y may be NULL).  Anything else: ADIL_EINVAL before any launch, outputs untouched.
 * Element offsets are 64-bit (m * ld).  One launch per call, no allocation; capturable. */
int adil_dense1x1_fwd_ld(const void* x, int ldx, const float* pscale, const float* pshift, const void* w,
                         const float* scale, const float* shift, void* y, int ldy,
                         int M, int K, int N, int act, void* stream);
int adil_dense1x1_bwd_ld(const void* g, int ldg, const void* y, int ldy, const float* scale, const void* wt,
                         const void* xin, int ldxin, const float* pscale, const float* pshift,
                         void* gx, int ldgx, int accumulate, int M, int K, int N, int act, void* stream);

/* 3x3 / stride 1 / pad 1 convolution with 32-channel granularity on either side, forward and input gradient: the growth
 * convolution (128 -> 32) behind every dense layer of the frozen DenseNet-121, which adil_conv3x3 (C % 64, N % 64) cannot
 * take.  Semantics of adil_conv3x3: channels_last bf16 storage, raw output, no epilogue.  In BOTH calls C is the layer's
 * input and N its output channel count, H x W the image:
 *   adil_dense3x3_fwd : y[B][H][W][N] = sum x[b][h+kh-1][w+kw-1][c] * w[n][c][kh][kw], zero padded;
 *                       wp [N][9][C] holds w[n][c][kh][kw] at [n][kh*3+kw][c]
 *   adil_dense3x3_bwd : gx[B][H][W][C] = sum g[b][h+1-kh][w+1-kw][n] * w[n][c][kh][kw];
 *                       wp_bwd [C][9][N] holds w[n][c][2-kh][2-kw] at [c][kh*3+kw][n]
 *                       (both layouts are those of adil_conv3x3: ops.pack_conv3x3_weights).  Input gradient only: the
 *                       network is frozen.
 * bf16 MFMA with fp32 accumulation in any order, ONE rounding to bf16 (nearest even), a zero sum written as +0.  A tap
 * that leaves the image (in the linear pixel tiling that includes a tap that would read the neighbouring image of the
 * batch) contributes nothing BY SELECTION, not by a multiplication with zero: a NaN or Inf in a neighbouring image does
 * not reach the output.  No atomics: bitwise reproducible.
 * Limits: C % 32 == 0, N % 32 == 0, 32 <= C, N <= 512, 1 <= W <= ADIL_DENSE3X3_MAX_W, H >= 1, B >= 1,
 * B H W <= 2^31 - 1, 16-byte aligned pointers.  Anything else, or a NULL pointer: ADIL_EINVAL before any launch, outputs
 * untouched.  No load or store leaves an operand's extent (the halo rows in front of the first and behind the last pixel
 * are read at clamped addresses and masked); every element of y / gx is written and nothing behind it.  Element offsets
 * are 64-bit.  One launch per call on `stream`, no allocation, no synchronisation, no zero-fill launch; capturable. */
#define ADIL_DENSE3X3_MAX_W 63
int adil_dense3x3_fwd(const void* x, const void* wp, void* y, int B, int H, int W, int C, int N, void* stream);
int adil_dense3x3_bwd(const void* g, const void* wp_bwd, void* gx, int B, int H, int W, int C, int N, void* stream);
/* The same two calls on pixel rows with a pitch: pixel m of x / g starts at base + m * ld (elements) and holds C / N live
 * channels, pixel m of y / gx likewise with N / C.  Nothing at or behind the width is read (halo rows included) or
 * written, so the 32-channel side can be a slice of a dense block's feature or gradient buffer.  wp / wp_bwd stay dense.
 * Limits of the plain calls, and ld >= width, ld % 8 == 0; else ADIL_EINVAL before any launch.  The plain calls are these
 * at ld = width (same launcher, same bits). */
int adil_dense3x3_fwd_ld(const void* x, int ldx, const void* wp, void* y, int ldy,
                         int B, int H, int W, int C, int N, void* stream);
int adil_dense3x3_bwd_ld(const void* g, int ldg, const void* wp_bwd, void* gx, int ldgx,
                         int B, int H, int W, int C, int N, void* stream);

/* A transition of the frozen DenseNet-121 — eval-BatchNorm + ReLU, 1x1 convolution, AvgPool2d(2, 2) — with the pooling done
 * IN FRONT of the convolution: the two commute, the GEMM runs on a quarter of the pixels and the full-resolution
 * convolution output is never written.  Forward and input gradient, one kernel each way.  channels_last bf16 storage:
 *     x, xin, gx     [B][H][W][K] bf16, dense
 *     y              [B][H/2][W/2][N] bf16, dense
 *     g              B H/2 W/2 pixel rows of N live elements at a row pitch of ldg ELEMENTS (the first channels of the next
 *                    dense block's gradient buffer are read in place); columns at or behind N are never read
 *     w              [N][K] bf16, wt [K][N] bf16 its transpose
 *     pscale, pshift [K] fp32 : the BatchNorm in front, as for adil_dense1x1_*
 *   Prologue : pre = fadd_rn(fmul_rn(f32(x), pscale[k]), pshift[k]), the two roundings of adil_dense1x1_* (never an fma);
 *              p = max(pre, 0) in fp32, every pre <= 0 or NaN gives +0; p is NOT rounded to bf16.
 *   Pooling  : output pixel (b, oh, ow) owns p00 = (2oh, 2ow), p01 = (2oh, 2ow+1), p10 = (2oh+1, 2ow), p11 = (2oh+1, 2ow+1);
 *              s = ((p00 + p01) + p10) + p11, three fp32 adds in this order, each rounded; a = bf16_rne(s * 0.25f).
 *   adil_dense_transition_fwd : y[b][oh][ow][n] = bf16_rne(sum_k a * w[n][k]), bf16 MFMA with fp32 accumulation in any
 *                       order.  No table and no activation behind the convolution: a transition has none.
 *   adil_dense_transition_bwd : t = sum_n g[mo][n] * wt[k][n] in fp32, any order, g used as stored; each of the four input
 *                       pixels of the window gets gx = bf16_rne(fmul(fmul(t, pscale[k]), 0.25f)) where THAT pixel's own
 *                       pre > 0, else +0; pre is recomputed from xin by the forward's two operations.  Every element of gx
 *                       is written.  Input gradient only: the network is frozen.
 * Limits: K % 8 == 0, N % 8 == 0, 8 <= K, N <= 2048, H and W even and >= 2, B >= 1, B H W < 2^31, ldg >= N, ldg % 8 == 0,
 * 16-byte aligned bf16 pointers, 4-byte aligned tables.  Anything else, or a NULL pointer: ADIL_EINVAL before any launch,
 * outputs untouched.  No load or store leaves an operand's extent: tails in K and N are clipped and zero-filled on BOTH MFMA
 * operands, pooled pixel rows past the end read a clamped in-range row and are not stored.  Element offsets are 64-bit.
 * One launch per call on `stream`, no allocation, no synchronisation.  No atomics: bitwise reproducible; capturable. */
int adil_dense_transition_fwd(const void* x, const float* pscale, const float* pshift, const void* w, void* y,
                              int B, int H, int W, int K, int N, void* stream);
int adil_dense_transition_bwd(const void* g, int ldg, const void* wt, const void* xin, const float* pscale,
                              const float* pshift, void* gx, int B, int H, int W, int K, int N, void* stream);

/* Whole-head self-attention of the frozen ViT-B/16 (head dimension 64), forward and input gradient, on the operands of the
 * two linear layers around it as they lie in memory, so no permute or reshape copy remains and no score matrix is written:
 *     qkv, gqkv [B][T][3][H][64] bf16 : the in-projection output [B][T][3 H 64]; q of head h at column h*64 + d, k at
 *                                       H*64 + h*64 + d, v at 2*H*64 + h*64 + d
 *     o, go     [B][T][H][64] bf16    : [B][T][H*64], what the out-projection reads
 *     lse       [B][H][T] fp32
 * For image b, head h, query i and key j < T:
 *     t_ij  = 0.125 * sum_d q_id k_jd          bf16 products, fp32 accumulation on the matrix pipe in any order; the
 *                                              factor 1/sqrt(64) is applied to the fp32 sum (exact)
 *     m_i   = max_j t_ij;  e_ij = exp(t_ij - m_i) in fp32 (hardware exp2 behind a multiplication with log2(e))
 *     l_i   = sum_j e_ij from the unrounded fp32 e;  lse_i = m_i + ln(l_i) in fp32 (natural logarithm)
 *     o_id  = bf16_rne((sum_j bf16_rne(e_ij) v_jd) / l_i)    the normalisation is ONE IEEE fp32 DIVISION on the accumulator
 *   adil_attn_bwd recomputes p_ij = exp(t_ij - lse_i), dp_ij = sum_d go_id v_jd, delta_i = sum_d f32(go_id) f32(o_id) from
 *   the stored bf16 o (fp32 fmas, d ascending in groups of 8, the 8 groups in a fixed tree), ds_ij = p_ij (dp_ij - delta_i)
 *   in fp32, and writes
 *     gv_jd = bf16_rne(sum_i bf16_rne(p_ij) go_id)
 *     gq_id = bf16_rne(0.125 * sum_j bf16_rne(ds_ij) k_jd)      gk_jd = bf16_rne(0.125 * sum_i bf16_rne(ds_ij) q_id)
 * Tiles are padded to 32 tokens inside the kernels: keys j >= T take no part in m, l, o, gq, gk or gv and query rows
 * i >= T add nothing to gk or gv, by SELECTION (p is set to zero there, never multiplied with a padded value).
 * One workgroup per (b, h) holds the head in LDS: 2 images of [T rounded up to 32][72] bf16 forward (36 KiB at T = 256),
 * 4 images and two fp32 vectors backward (146 KiB at T = 256 of the CU's 160 KiB), which sets adil_attn_max_tokens() = 256.
 * Limits: 1 <= T <= adil_attn_max_tokens(), H >= 1, B >= 1, B * H <= 2^31 - 1 (the (image, head) pair is the grid's x
 * index), 16-byte aligned pointers.  Anything else, or a NULL pointer: ADIL_EINVAL before any launch, outputs untouched.
 * Every element of o, lse and gqkv is written and nothing behind them; no load or store leaves an operand's extent.
 * Element offsets are 64-bit.  One launch per call on `stream`, no allocation, no synchronisation.  No atomics: bitwise
 * reproducible across calls and processes; capturable.  Behaviour for non-finite inputs is not promised beyond the rule
 * that no access leaves the extents. */
int adil_attn_max_tokens(void);
int adil_attn_fwd(const void* qkv, void* o, float* lse, int B, int T, int H, void* stream);
int adil_attn_bwd(const void* qkv, const void* o, const float* lse, const void* go, void* gqkv, int B, int T, int H,
                  void* stream);

/* adil_conv3x3 for ANY width (the 3x3 convolutions of a frozen VGG; added under ABI 8 like the entry points above):
 * exactly its contract — channels_last bf16 x[B][H][W][C], weights wp[N][9][C] of the same two packs, raw bf16
 * y[B][H][W][N], the input gradient the same call on the flipped pack with C and N exchanged, bf16 MFMA products with
 * fp32 accumulation and one RNE rounding (a zero sum is written as +0) — on 2-D pixel tiles inside one image (8 x 16
 * pixels x 128 channels where N % 128 == 0, else 16 x 16 x 64) instead of linear ones.  A halo pixel outside the image is
 * staged as zeros by selection; its load goes to the nearest pixel of the same image, so nothing of a neighbouring image or
 * outside the operand is read and a NaN or Inf next door never meets a multiplier.  Per accumulator the MFMAs run in
 * adil_conv3x3's order (chunk -> tap -> k), so both give the same bits where both accept the shape.
 * Limits: C % 64 == 0, N % 64 == 0, B, H, W >= 1 (any W), B * H * W < 2^31, 9 * C * N < 2^31, non-null 16-byte aligned
 * pointers; anything else ADIL_EINVAL before any launch, outputs untouched.  One launch on `stream`, no allocation, no
 * atomics (bitwise reproducible), capturable, 64-bit element offsets; every element of y is written, nothing behind it. */
int adil_conv3x3_wide(const void* x, const void* wp, void* y, int B, int H, int W, int C, int N, void* stream);

/* bias + ReLU + 2x2 / stride 2 max-pool behind a raw convolution output, and its input gradient (added under ABI 8):
 *     x, gx [B][H][W][C] bf16      bias [C] fp32 or NULL      y, g [B][H/2][W/2][C] bf16      idx [B][H/2][W/2][C] uint8
 * Forward, per window and channel: t = fp32(x) + bias[c] (one fp32 add); the winner is the first of (0,0), (0,1), (1,0),
 * (1,1) that is strictly greater than all before it; y = bf16_rne(max(t_winner, 0)) with a zero written as +0;
 * idx = dh * 2 + dw of the winner, or 4 where t_winner <= 0 (a dead window).  Backward: gx at the winner's position takes
 * the bits of g, every other element — all four of a dead window — is +0, and every element of gx is written.  That is
 * torch's fp32 chain max_pool2d(relu(x.float() + bias), 2) and its autograd bit for bit, ties included.
 * Limits: H, W even, C % 8 == 0, B, H, W, C >= 1, B * H * W < 2^31, non-null pointers aligned to 16 bytes (idx: 8);
 * anything else ADIL_EINVAL before any launch, outputs untouched.  One launch each, no allocation, no atomics,
 * capturable, 64-bit element offsets. */
int adil_bias_relu_pool2_fwd(const void* x, const float* bias, void* y, void* idx, int B, int H, int W, int C, void* stream);
int adil_bias_relu_pool2_bwd(const void* g, const void* idx, void* gx, int B, int H, int W, int C, void* stream);

/* The first group of a frozen VGG11 — Normalize, conv 3 -> 64 (3x3, stride 1, pad 1, bias), ReLU, MaxPool2d(2, 2) — as one
 * kernel each way on the attack's own tensors (added under ABI 8).  The 64-channel tensor at H x W never reaches memory.
 *     x, gx [B][3][H][W] NCHW, fp32 or bf16 (x_dtype / gx_dtype: ADIL_F32 / ADIL_BF16), as in adil_first3x3_fwd / _bwd
 *     y, g  [B][H/2][W/2][64] bf16 channels_last      idx [B][H/2][W/2][64] uint8, the format of adil_bias_relu_pool2_*
 *     w_fwd [64][3][4][4] bf16 = w[n][c][kh][kw] at [n][kh][kw][c], zero for kw = 3 / c = 3
 *     w_bwd [3][9][64] bf16 = w[n][c][kh][kw] at [c][kh*3+kw][n] (channels swapped, taps NOT flipped)      bias [64] fp32
 * Forward:
 *     x' = bf16( f32( f32(x - mean[c]) * inv_std[c] ) ): the subtraction and the product each rounded to fp32 on its own
 *          (no contraction), then one RNE rounding; the zero padding is applied to x', the NORMALISED tensor.
 *     s  = sum over the 27 taps of x' * w: bf16 MFMA products (exact in fp32), fp32 accumulation, one instruction per tap
 *          row kh with the K order (kw, c).
 *     t  = s + bias[n]: one fp32 add, no bf16 rounding in between.
 *     The winner of a 2x2 window is the first of (0,0), (0,1), (1,0), (1,1) that is strictly greater than all before it,
 *     compared on the fp32 t; y = bf16_rne(max(t_winner, 0)) with a zero written as +0; idx = 2 dh + dw of the winner, or
 *     4 where t_winner <= 0 (a dead window).
 * Backward (needs neither x nor y):
 *     gz[h][w][n] takes the bits of g[h/2][w/2][n] where idx[h/2][w/2][n] == 2 (h & 1) + (w & 1), else +0; it is formed
 *     while g is staged in LDS and never written to memory.
 *     gx[c][h][w] = round( inv_std[c] * sum_{kh,kw,n} gz[h+1-kh][w+1-kw][n] * w[n][c][kh][kw] ): per accumulator the taps in
 *     the order kh*3+kw, within a tap channels 0..31 in one MFMA before 32..63 in the next; the product with inv_std is
 *     one fp32 operation, then the rounding to the storage type.
 * Limits: H, W even and >= 2, 1 <= B <= 65535 (the image index is a grid dimension), B * H * W < 2^31, dtype ADIL_F32 or
 * ADIL_BF16, non-null pointers aligned to 16 bytes (x, gx: their element size; idx of the backward: 8); anything else
 * ADIL_EINVAL before any launch, outputs untouched.  Out-of-range positions are never loaded (predicated), so nothing of
 * a neighbouring image is read and a NaN in one image never reaches another.  One launch each on `stream`, no allocation,
 * no synchronisation, no atomics (bitwise reproducible), capturable, 64-bit element offsets; every element of y, idx and
 * gx is written, nothing behind them. */
int adil_first3x3_pool_fwd(const void* x, int x_dtype, const void* w_fwd, float mean0, float mean1, float mean2,
                           float inv_std0, float inv_std1, float inv_std2, const float* bias, void* y, void* idx, int B,
                           int H, int W, void* stream);
int adil_first3x3_pool_bwd(const void* g, const void* idx, const void* w_bwd, float inv_std0, float inv_std1,
                           float inv_std2, void* gx, int gx_dtype, int B, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADIL_HIP_H */
