// adil_first_patch.h — what the kernels on the attack's own [B][3][H][W] tensors share: stem_conv_fwd_kernel /
// stem_conv_bwd_shift_kernel (adil_stem.hip), first3x3_fwd_kernel / first3x3_bwd_kernel (adil_first_conv.hip) and
// first3x3_pool_fwd_kernel / first3x3_pool_bwd_kernel (adil_vgg_first.hip).
//
// first3x3_fwd_kernel and first3x3_pool_fwd_kernel stage the same normalised patch (predicated NCHW loads of three planes,
// (x - mean) * inv_std under fp contract(off), zeros outside the image, pack to [row][col][4 ch]) and the two gradients end in
// the same predicated three-plane `acc * inv_std` store.  Those stay written out in the four kernels: as __forceinline__
// helpers (two staging phases and a store) they kept every register count and occupancy but not the assembly (hipcc
// optimises a helper on its own before it inlines it), and a changed kernel has to be timed before it may stay
// (profiles/conv3x3_one_kernel.md).  A change to one copy goes to the other.
#pragma once

namespace {

struct InputNorm { float mean[3]; float inv_std[3]; };   // Normalize as the kernels take it: (x - mean) * inv_std

typedef float f32x4 __attribute__((ext_vector_type(4)));

}  // namespace
