// Shared definitions of the fp8 P.V attention (attention_fp8.hip): the private layout of the quantised V that the V quantiser
// writes and the attention kernel reads, defined once here for both.
//
// Keys are taken in STEPS of 128, the reduction length of one v_mfma_scale_f32_16x16x128_f8f6f4.  Within a step the score MFMA
// (v_mfma_f32_16x16x32_f16, S^T = K Q^T, 8 key blocks of 16) leaves lane (query i16, group g = lane >> 4) holding register r of key
// block kb for key 16 kb + 4 g + r.  Packed to e4m3 as they sit, those 32 values are the lane's B operand of the P.V MFMA, byte
// j = 4 kb + r.  So the kappa order of a step is
//     position p = 32 g + 4 kb + r  <->  key 16 kb + 4 g + r          (pv8_key_of)
// and V^T is stored in it: lane (dim i16 of a 16-dim block, g) of the A operand reads 32 consecutive bytes, positions [32 g, 32 g + 32).
// The MFMA sees byte j of lane group g as reduction index k = 64 (j >> 4) + 16 g + (j & 15), and it applies the E8M0 scale of lane
// (row, b) to k in [32 b, 32 b + 32) (measured: the lane's own 32 bytes are NOT its scale block).  So scale group b of a channel is
// the 32 positions 32 g + 16 (b >> 1) + jj, g in {2 (b & 1), 2 (b & 1) + 1}, jj < 16 (pv8_group_pos): one E8M0 byte per (step,
// group b, channel).  Steps are per sample (a (batch, head) pair has ceil(lk / 128) of them, keys >= lk zero-padded), so no group
// straddles two scenes.
//
// Global image of one (batch, head, step):
//   values: 64 rows (channels) x 128 bytes (positions), 16-byte chunk c of row d stored at chunk c ^ ((d >> 1) & 7) -- the LDS image
//           itself (copied by LDS-DMA as is); the 16 lanes of a ds_read_b128 read 16 rows of one chunk column without bank conflicts
//   scales: 256 bytes, byte 4 (16 b + (d & 15)) + (d >> 4) = 127 + e of (channel d, group b): lane (i16, g = b) reads ONE dword whose
//           byte db is the scale of its row's block b in 16-dim block db (the OPSEL of the block-scaled MFMA)
// Values of a group are e4m3(v * 2^-e), saturating, round-to-nearest-even, e the smallest integer with max|v| * 2^-e <= 448
// (seva.ops.quantize_weight_fp8's rule, evaluated exactly), clamped to [-126, 127]; an all-zero group gets the rule applied to 1e-30.
#pragma once

#include "seva_common.h"

#define PV8_STEP 128           // keys per step (one scaled MFMA)
#define PV8_VALUE_BYTES 8192   // 64 channels x 128 keys per (batch, head, step)
#define PV8_SCALE_BYTES 256    // 64 channels x 4 groups

__host__ __device__ __forceinline__ int pv8_key_of(int pos) { return 16 * ((pos >> 2) & 7) + 4 * (pos >> 5) + (pos & 3); }
__host__ __device__ __forceinline__ int pv8_chunk_swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }
// position of element j (0 .. 31) of scale group b
__host__ __device__ __forceinline__ int pv8_group_pos(int b, int j) { return 32 * (2 * (b & 1) + (j >> 4)) + 16 * (b >> 1) + (j & 15); }
__host__ __device__ __forceinline__ int pv8_scale_index(int dim, int group) { return 4 * (16 * group + (dim & 15)) + (dim >> 4); }
__host__ __device__ __forceinline__ int pv8_steps(int lk) { return (lk + PV8_STEP - 1) / PV8_STEP; }
