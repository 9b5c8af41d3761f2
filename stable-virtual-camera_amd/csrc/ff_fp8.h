// Shared definitions of the e4m3 fused feed-forward (ff_fused.hip: ff_fused8_fp8_kernel, seva_ff_fused_fp8): the private
// weight layouts that seva.ops.pack_ff_fp8 writes and the kernel reads, defined once here.
//
// W1: [8C][KP] e4m3 bytes, KP = the multiple of 128 at or above C (64 -> 128, 320 -> 384), columns >= C zero; rows in the
//     interleaved GEGLU order of seva_gemm_f16 (groups of 64 = [32 value | 32 gate]); w1_exp[8C] = 127 + e of each row.
//
// W2: [C][4C] e4m3 bytes, w2_exp[C].  The hidden features are taken in STEPS of 128 (one v_mfma_scale_f32_16x16x128_f8f6f4 k-step
// = two 64-feature chunks c = 0, 1 of stage 1).  After stage 1 of a step, wave half q (0, 1) of a row group holds in lane group g
// the features 64 c + 32 q + 8 g + r (r < 8) of each of its tokens -- the paired row assignment of gemm.hip -- and the B operand
// of the step's MFMA for lane group g is [the 16 bytes of half 0 | the 16 bytes of half 1], byte order (c, r) within each.
// The weight operand of lane group g is chunks g (lo) and 4 + g (hi) of a 128-byte row slice, like every other fp8 operand
// of the library.  So byte P of a row's step slice holds feature
//     ff8_feature_of(P) = 64 c + 32 q + 8 g + r,   P = 64 q + 16 g + 8 c + r
// and W2 is stored column-permuted:  W2_stored[n][128 s + P] = W2[n][128 s + ff8_feature_of(P)].  The k order the MFMA itself
// assigns to (lane group, byte) does not matter: both operands use the same (lane group, byte) -> feature map, and the weight
// scale is constant along K.
#pragma once

#define FF8_STEP 128                              // hidden features per stage-2 k-step
#define FF8_KP(C) (((C) + 127) / 128 * 128)       // W1 row length in bytes (stage-1 reduction, zero-padded)

__host__ __device__ __forceinline__ int ff8_feature_of(int pos) {
  return 64 * ((pos >> 3) & 1) + 32 * (pos >> 6) + 8 * ((pos >> 4) & 3) + (pos & 7);
}
