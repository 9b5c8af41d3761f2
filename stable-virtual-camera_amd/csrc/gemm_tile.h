// The tile core of gemm.hip, conv_win.hip and ff_fused.hip (through gemm_common.h; the last two write it out).  An operand row of a K-tile (64 f16 or
// 128 e4m3 elements) is 128 bytes of LDS = 8 chunks of 16 bytes, staged by LDS-DMA 8 rows per wave-instruction (lane: row lane >> 3,
// physical chunk sp = lane & 7).  The image is lane-linear; the bank-conflict swizzle (logical chunk c of row r at physical chunk
// c ^ key(r)) is applied on the per-lane SOURCE address and again on the ds_read_b128 fragment reads.  The MFMA takes the WEIGHT fragment
// as its A operand, so lane (fr = lane & 15, fg = lane >> 4) holds 4 consecutive output features (rows of D) of token row fr.
// What keeps hipcc's output what it was (checked per instantiation: tools/codegen_diff.py, profiles/gemm_tile_refactor.log, which also
// lists what was tried and stays written out per kernel): __forceinline__ everywhere, register arrays BY REFERENCE TO ARRAY, `#pragma
// unroll` inside the helper, constexpr int arithmetic in the association the kernels had, lane / wave values taken from the kernel.
#pragma once

#define SEVA_TILE_FN __host__ __device__ __forceinline__ constexpr

// natural key: the 16 rows r0 .. r0 + 15 of an MFMA block are read together; bits {1, 2, 3} of the row
SEVA_TILE_FN int key_nat(int row) { return (row >> 1) & 7; }
// paired key (WRowMap, PAIRED): the rows read together are 8 (fr >> 2) + (fr & 3) of a 32-row pair region; bits {1, 3, 4} of the row
SEVA_TILE_FN int key_pair(int row) { return ((row >> 1) & 1) | (((row >> 3) & 3) << 1); }
// logical chunk that the staging lane of physical chunk sp fetches for a row with swizzle key `key`
SEVA_TILE_FN int src_chunk(int sp, int key) { return sp ^ key; }
// byte offset, inside a tile of 128-byte rows, of lane group fg's fragment of k-step s (logical chunk 4 s + fg) in `row`
SEVA_TILE_FN int frag_off(int row, int key, int s, int fg) { return row * 128 + (((4 * s + fg) ^ key) << 4); }

namespace tile_check {
constexpr int pair_row(int fr) { return 8 * (fr >> 2) + (fr & 3); }
// per row a bijection of the 8 chunks; over the 16 rows read together two rows per physical chunk; a paired block's offset keeps the key
template <bool PAIR>
constexpr bool key_ok() {
  for (int base = 0; base < 320; base += PAIR ? 4 : 16) {  // PAIR: every block start 32 p + 4 e
    if (PAIR && (base & 31) != 0 && (base & 31) != 4) continue;
    int uses[8] = {};
    for (int fr = 0; fr < 16; ++fr) {
      const int row = base + (PAIR ? pair_row(fr) : fr), key = PAIR ? key_pair(row) : key_nat(row);
      int seen = 0;
      for (int c = 0; c < 8; ++c) seen |= 1 << src_chunk(c, key);
      if (seen != 0xFF || (PAIR && key != key_pair(pair_row(fr)))) return false;  // (PAIR: the block offset 32 p + 4 e leaves the key alone)
      ++uses[key];
    }
    for (int k = 0; k < 8; ++k)
      if (uses[k] != 2) return false;
  }
  return true;
}
}  // namespace tile_check
static_assert(tile_check::key_ok<false>() && tile_check::key_ok<true>(), "chunk swizzle: bijection per row, two rows per chunk per read, block-invariant paired key");

// D row r of a 16-row block lands in lane group fg = r >> 2.  Natural order: block j reads rows 16 j + r, a lane owns 4 consecutive
// features per block, 16 apart.  PAIRED: blocks are taken in pairs (2p, 2p + 1) over 32 weight rows and MFMA row r of block 2p + e
// reads row 32 p + 8 (r >> 2) + 4 e + (r & 3), so lane group fg owns the 8 consecutive features 32 p + 8 fg .. + 7 across the pair
// (one 16-byte f16 store; the B operand fragment of the next MFMA in ff_fused.hip).  An odd last block keeps the natural order.
template <int NJ, bool PAIRED>
struct WRowFns {
  static constexpr int NJP = PAIRED ? (NJ & ~1) : 0;  // blocks handled in pairs
  // first feature (= weight row, relative to the wave's first) of block j for lane group fg
  static SEVA_TILE_FN int feat_of(int j, int fg) { return j < NJP ? 32 * (j >> 1) + 8 * fg + 4 * (j & 1) : 16 * j + 4 * fg; }
  // weight row that MFMA row r of block j reads: feat_of(j, r >> 2) + (r & 3) (wrow_map_ok), in the association the kernels had
  static SEVA_TILE_FN int wrow_of(int j, int r) { return j < NJP ? 32 * (j >> 1) + 4 * (j & 1) + 8 * (r >> 2) + (r & 3) : 16 * j + r; }
  // = (lane's row in block 0) + (row offset of block j) for all but an odd last block of a paired map; the offset keeps the key
  static SEVA_TILE_FN int lane_row(int fr) { return wrow_of(0, fr); }
  static SEVA_TILE_FN int block_row(int j) { return feat_of(j, 0); }
  // swizzle key of wave-relative row rw: follows the rows read together
  static SEVA_TILE_FN int key(int rw) { return rw < NJP * 16 ? key_pair(rw) : key_nat(rw); }
};
template <int NJ, class F>
constexpr bool wrow_map_ok() {
  bool seen[16 * NJ] = {};
  for (int j = 0; j < NJ; ++j)
    for (int r = 0; r < 16; ++r) {
      const int w = F::wrow_of(j, r);
      if (w < 0 || w >= 16 * NJ || seen[w] || w != F::feat_of(j, r >> 2) + (r & 3)) return false;
      if (w != (j < F::NJP || F::NJP == 0 ? F::lane_row(r) + F::block_row(j) : 16 * j + r)) return false;  // (odd last block: natural)
      seen[w] = true;
    }
  return true;
}
template <int NJ, bool PAIRED>
struct WRowMap : WRowFns<NJ, PAIRED> {
  static_assert(wrow_map_ok<NJ, WRowFns<NJ, PAIRED>>(), "wrow_of: a permutation of the wave's 16 NJ rows, block offset + lane row");
};

// an empty asm "rewrites" every element in place: retires loads before a counted-vmcnt loop, keeps a K-tile's MFMAs before its barrier
template <class T, int N>
__device__ __forceinline__ void pin_regs(T (&x)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" : "+v"(x[i]));
}
template <class T, int M, int N>
__device__ __forceinline__ void pin_regs(T (&x)[M][N]) {
#pragma unroll
  for (int i = 0; i < M; ++i) pin_regs(x[i]);
}

// one k-step of 32 of a K-tile's f16 product: af[i] = fragment of token block i, bf[j] = fragment of weight block j (the MFMA's A operand)
template <int MI, int NJ>
__device__ __forceinline__ void mfma_step_f16(f32x4 (&acc)[MI][NJ], const half8_t (&af)[MI], const half8_t (&bf)[NJ]) {
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j], af[i], acc[i][j], 0, 0, 0);
}
