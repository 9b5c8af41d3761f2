// Scaffolding shared by the flash-attention kernels of attention.hip (attn_kernel, attn2_kernel, attn16_kernel) and attention_fp8.hip
// (pv8_kernel): which (batch, head, query block, key range) a workgroup owns, the 3-deep LDS-DMA ring of K/V tiles and the pieces of
// the loop that drives it, the output epilogue, and the host-side descriptor checks.  A kernel is its own arithmetic (scores, softmax,
// P.V) written as a tile body against these.  Everything on the device side is inlined into the kernel; nothing goes through memory.
// hipcc's register allocation of these kernels follows the FORM of this code (profiles/attn_common_refactor.log): helpers fill structs
// by reference instead of returning them, and take the kernel's own lane / wave / i16 / g instead of deriving them from threadIdx.x
// again.  Compare the emitted code of every instantiation after a change here.
#pragma once

#include <initializer_list>
#include <type_traits>

#include "seva_common.h"

// ---- arguments ----------------------------------------------------------------------------------------------------------------
// What every kernel takes.  attention.hip's kernels take it as it is; Pv8Args derives from it and adds its quantised V.  (The order of
// the fields is the kernels' kernarg layout, which hipcc's scalar-load grouping and with it the SGPR counts depend on.)
struct AttnBase {
  const half_t* q;
  const half_t* k;
  const half_t* v;  // f16 V with K's strides (null for the fp8 P.V kernel)
  half_t* out;
  int64_t q_sb0, q_sb1, q_sl;
  int64_t k_sb0, k_sb1, k_sl;
  int64_t o_sb0, o_sb1, o_sl;
  int32_t nb1, heads, lq, lk, qblocks;
  float scale_log2;  // softmax scale * log2(e)  (unused when q is pre-scaled)
  int32_t dbg;       // ablation bits (SEVA_ATTN_DBG; timing only): 1 no K/V reloads, 2 no softmax, 4 no P*V, 8 no Q*K
  // K/V split (SPLIT instantiations + attn_combine_kernel): every (batch, head, query block) is computed by `nsplit` workgroups,
  // each over a contiguous range of whole K/V tiles, which leave their UN-normalised fp32 O rows and (m, l) in the workspace
  float* part_o;   // [nsplit][batch * heads * lq][64]
  float* part_ml;  // [nsplit][batch * heads * lq][2]
  int32_t nsplit;
};

// K tile in LDS: 128-byte rows, 16-byte chunk c of row r stored at c ^ ((r >> 1) & 7) (conflict-free b128 row reads).  The V swizzle
// is the kernel's (it follows the MFMA shape of its P.V product) and is handed to the ring as a template parameter.
__device__ __forceinline__ int k_chunk_swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }
typedef int (*attn_swz_t)(int row, int chunk);

// ---- workgroup decode -----------------------------------------------------------------------------------------------------------
// logical id = (((batch * heads) + head) [* nsplit + split]) * qblocks + qblock.  Hardware deals blocks b, b+8, ... to one XCD; the
// bijective remap gives every XCD one contiguous run of logical ids, so the q-blocks of a (batch, head[, split]) -- which all stream
// the same K/V -- share one L2.
__device__ __forceinline__ int attn_xcd_remap() {
  const int nb = gridDim.x, q = nb >> 3, r = nb & 7, x = blockIdx.x & 7;
  return ((x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (blockIdx.x >> 3);
}

struct AttnWg {
  int qb, ksp, head, batch, b0, b1;
  int key0, lk;  // this workgroup's key range [key0, key0 + lk): the whole sequence, or the split's run of whole tiles
};
template <bool SPLIT>
__device__ __forceinline__ void attn_decode(const AttnBase& p, int KT, AttnWg& w) {
  int bid = attn_xcd_remap();
  w.qb = bid % p.qblocks;
  bid /= p.qblocks;
  w.ksp = 0;
  if (SPLIT) {
    w.ksp = bid % p.nsplit;
    bid /= p.nsplit;
  }
  w.head = bid % p.heads;
  w.batch = bid / p.heads;
  w.b0 = w.batch / p.nb1;
  w.b1 = w.batch - w.b0 * p.nb1;
  w.key0 = 0;
  w.lk = p.lk;
  if (SPLIT) {
    const int nt_all = (p.lk + KT - 1) / KT, tps = (nt_all + p.nsplit - 1) / p.nsplit;
    w.key0 = w.ksp * tps * KT;
    const int key1 = (w.ksp + 1) * tps * KT < p.lk ? (w.ksp + 1) * tps * KT : p.lk;
    w.lk = key1 - w.key0;  // > 0: the host only splits when every split gets at least one tile
  }
}
__device__ __forceinline__ const half_t* attn_q_base(const AttnBase& p, const AttnWg& w) {
  return p.q + w.b0 * p.q_sb0 + w.b1 * p.q_sb1 + w.head * 64;
}
// first key of the workgroup's range in K (or in a V with K's strides)
__device__ __forceinline__ const half_t* attn_kv_base(const AttnBase& p, const AttnWg& w, const half_t* kv) {
  return kv + w.b0 * p.k_sb0 + w.b1 * p.k_sb1 + w.head * 64 + (int64_t)w.key0 * p.k_sl;
}
__device__ __forceinline__ half_t* attn_o_base(const AttnBase& p, const AttnWg& w) {
  return p.out + w.b0 * p.o_sb0 + w.b1 * p.o_sb1 + w.head * 64;
}

// Tell hipcc's wait-count bookkeeping that the loads into these registers have landed (no instruction is emitted).
__device__ __forceinline__ void attn_retire_loads(half8_t& v) { asm volatile("" : "+v"(v)); }
template <class T, int N>
__device__ __forceinline__ void attn_retire_loads(T (&a)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) attn_retire_loads(a[i]);
}

// ---- K/V ring ---------------------------------------------------------------------------------------------------------------------
// 3-deep ring of tiles in LDS, [buf][K tile | V tile | ...], filled by LDS-DMA two tiles ahead.  Each of the NW waves copies IP 8-row
// slabs of K (and, with a V swizzle, of an f16 V with K's strides; VSWZ = nullptr: K only, the kernel copies its own V) per tile:
// lane (r = lane >> 3, physical chunk = lane & 7) of each 8-row wave-instruction; the swizzle is applied on the SOURCE chunk (the LDS
// image of an LDS-DMA is lane-linear).
// Tiles are issued strictly in order 0, 1, 2, ...: the per-lane source pointers of the NEXT tile to issue are running state, advanced
// by the workgroup-uniform tile stride (the 64-bit key * stride products cost four quarter-rate v_mul_lo_u32 / two v_mad_u64_u32 per
// tile in a VALU-bound kernel).  Only a partial last tile recomputes its addresses, to clamp the rows past lk onto the last key
// (their scores are masked).
template <int KT, int NW, int BUF_BYTES, attn_swz_t VSWZ>
struct AttnRing {
  static constexpr bool HAS_V = VSWZ != nullptr;
  static constexpr int IP = KT / 8 / NW;         // 8-row LDS-DMA instructions per wave per operand per tile
  static constexpr int G = (HAS_V ? 2 : 1) * IP;  // ... per wave per tile
  static_assert(KT % (8 * NW) == 0, "tile rows must split over the waves");

  const half_t* kbase;
  const half_t* vbase;
  int64_t k_sl;
  int lk;
  int64_t tile_stride;
  int nt, wave_u, sr, sp;
  unsigned smem_base;
  bool ragged;
  const half_t* kp[IP];
  const half_t* vp[HAS_V ? IP : 1];

  // kbase / vbase: first key of the range (attn_kv_base), lk keys; smem: the ring; lane, wave: the kernel's own (hipcc turns a second
  // readfirstlane(threadIdx.x >> 6) into readfirstlane(threadIdx.x) >> 6, and everything derived from it changes)
  __device__ __forceinline__ AttnRing(const half_t* kbase_, const half_t* vbase_, int64_t k_sl_, int lk_,
                                      const char* smem, int lane, int wave)
      : kbase(kbase_), vbase(vbase_), k_sl(k_sl_), lk(lk_) {
    nt = (lk + KT - 1) / KT;
    wave_u = __builtin_amdgcn_readfirstlane(wave);
    smem_base = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)smem);
    sr = lane >> 3, sp = lane & 7;
#pragma unroll
    for (int i = 0; i < IP; ++i) {
      const int row = 8 * (wave_u * IP + i) + sr;
      const int key = row < lk ? row : lk - 1;
      kp[i] = kbase + (int64_t)key * k_sl + k_chunk_swz(row, sp) * 8;
      if constexpr (HAS_V) vp[i] = vbase + (int64_t)key * k_sl + VSWZ(row, sp) * 8;
    }
    tile_stride = (int64_t)KT * k_sl;
    ragged = (lk % KT) != 0;
  }
  __device__ __forceinline__ void operator()(int kt, int buf) {
    const bool clamp = ragged && kt == nt - 1 && kt > 0;  // (tile 0 was clamped when the pointers were built)
#pragma unroll
    for (int i = 0; i < IP; ++i) {
      const unsigned dst = smem_base + buf * BUF_BYTES + 8 * (wave_u * IP + i) * 128;
      if (clamp) {
        const int row = 8 * (wave_u * IP + i) + sr;
        int key = kt * KT + row;
        if (key >= lk) key = lk - 1;
        const int64_t roff = (int64_t)key * k_sl;
        glds16_raw(kbase + roff + k_chunk_swz(row, sp) * 8, dst);
        if constexpr (HAS_V) glds16_raw(vbase + roff + VSWZ(row, sp) * 8, dst + KT * 128);
      } else {
        glds16_raw(kp[i], dst);
        if constexpr (HAS_V) glds16_raw(vp[i], dst + KT * 128);
      }
      kp[i] += tile_stride;
      if constexpr (HAS_V) vp[i] += tile_stride;
    }
  }
};

// The ring driver.  A kernel declares its tile body, then starts the ring and walks the tiles:
//     auto tile = [&](int buf, auto masked_c, int kt) {
//       ... smem + buf * BUF_BYTES is tile kt ...
//       const bool more2 = attn_ring_prefetch(kt, nt, buf, true, issue);
//       ... scores, softmax, P.V ...
//       attn_ring_arrive<G>(more2);
//     };
//     attn_ring_start<G>(nt, issue, qf);
//     const int nfull = lk / KT;  // tiles that need no mask (the ragged tail tile, if any, is the last one)
//     int buf = 0;                // buffer index == tile % 3
//     for (int kt = 0; kt < nfull; ++kt) {
//       tile(buf, std::false_type{}, kt);
//       buf = buf == 2 ? 0 : buf + 1;
//     }
//     if (nfull < nt) tile(buf, std::true_type{}, nfull);
// `issue(kt, buf)` starts tile kt's copies into buffer buf with G LDS-DMA instructions per wave: an AttnRing, or a kernel's lambda around
// one.  (The loop itself stays in the kernel: moved into a function here, hipcc orders attn_kernel<1, 32>'s LDS address arithmetic
// differently and its tile loop grows by two VALU instructions; the pieces below leave every kernel's loop as it was.)
//  * MASKED = decltype(masked_c)::value is compile-time so that the tail mask costs nothing on full tiles.
//  * The buffer index is a RUN-TIME (wave-uniform) value: with the three buffers as three unrolled copies of the body hipcc gave the
//    loop-carried O accumulators different registers in different copies and moved all 32 of them (16 v_mov_b64 behind two `s_nop 11`
//    MFMA-result hazards) in every tile, and rebuilt the 16-register splat of -m_run; one body has one assignment.

// Prologue: tiles 0 and 1 are issued, tile 0 has landed.  The kernel's Q fragment registers `qf` are retired HERE, after the waits and
// before the first barrier, as far as hipcc's wait-count bookkeeping is concerned.  Otherwise they are "possibly pending" at the loop
// header (merged over the back-edge), the compiler guards the first use of the Q registers in EVERY tile with s_waitcnt vmcnt(3) ..
// vmcnt(0), and that vmcnt(0) drains the LDS-DMA ring (which it cannot see: the DMAs are issued from inline asm) once per tile.
template <int G, class Issue, class QF>
__device__ __forceinline__ void attn_ring_start(int nt, Issue&& issue, QF& qf) {
  issue(0, 0);
  if (nt > 1) {
    issue(1, 1);
    wait_vm<G>();
  } else {
    wait_vm<0>();
  }
  attn_retire_loads(qf);
  __syncthreads();
}
// Top of tile kt in buffer buf: tile kt+2 goes to buffer (kt+2)%3, last read in iteration kt-1 (every wave passed that barrier).
// reload = false stops the copies after the prologue (ablation, timing only).  Returns whether a tile was issued.
template <class Issue>
__device__ __forceinline__ bool attn_ring_prefetch(int kt, int nt, int buf, bool reload, Issue&& issue) {
  const bool more2 = kt + 2 < nt && reload;
  if (more2) issue(kt + 2, buf == 0 ? 2 : buf - 1);  // (buf + 2) % 3
  return more2;
}
// End of tile kt: tile kt+1 (issued one iteration ago) must have landed; tile kt+2's G instructions may fly on
template <int G>
__device__ __forceinline__ void attn_ring_arrive(bool more2) {
  if (more2) wait_vm<G>();
  else wait_vm<0>();
  __syncthreads();
}

// ---- epilogue ---------------------------------------------------------------------------------------------------------------------
// O goes through LDS so that every global store is a full 128-byte row (per-lane 8-byte stores at a row stride touch 32 lines per
// instruction and amplify HBM writes; profiles/r01_traffic.json).  Each wave owns an image of 128-byte rows in the (idle) K/V buffers
// -- callers put a __syncthreads() between the last tile and the first stage call -- where 16-byte chunk c of row r sits at c ^ (r & 7).
// four consecutive head dims d0 .. d0 + 3 of image row `row`, normalised:
__device__ __forceinline__ void attn_stage_o4(char* ow, int row, int d0, f32x4 o, float inv) {
  half4_t h;
#pragma unroll
  for (int r = 0; r < 4; ++r) h[r] = (half_t)(o[r] * inv);
  const int chunk = d0 >> 3, piece = (d0 >> 2) & 1;  // 16-byte chunk, 8-byte half
  *(half4_t*)(ow + row * 128 + ((chunk ^ (row & 7)) << 4) + (piece << 3)) = h;
}
// a 32-query block of v_mfma_f32_32x32x16 accumulators: lane (qi = lane & 31, hh = lane >> 5) holds dims 32 db + 8 t + 4 hh .. + 3 of
// query qi in acc[db][4 t .. 4 t + 3]
__device__ __forceinline__ void attn_stage_o32(char* ow, int qi, int hh, const f32x16 (&acc)[2], float inv) {
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int t = 0; t < 4; ++t)
      attn_stage_o4(ow, qi, 32 * db + 8 * t + 4 * hh, f32x4{acc[db][4 * t], acc[db][4 * t + 1], acc[db][4 * t + 2], acc[db][4 * t + 3]}, inv);
}
// The wave reads back its own image (no workgroup barrier needed, only the LDS round trip) and stores PASSES x 8 rows, query rows
// q0, q0 + 1, ... of the workgroup's (batch, head), those below lq.
template <int PASSES>
__device__ __forceinline__ void attn_store_rows(const char* ow, half_t* obase, int64_t o_sl, int q0, int lq, int lane) {
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < PASSES; ++i) {
    const int row = 8 * i + (lane >> 3), pchunk = lane & 7;
    const uint4 v = *(const uint4*)(ow + row * 128 + (pchunk << 4));
    const int lchunk = pchunk ^ (row & 7);
    if (q0 + row < lq) *(uint4*)(obase + (int64_t)(q0 + row) * o_sl + lchunk * 8) = v;
  }
}
// row of this workgroup's (split, batch, head) in the K/V-split workspace, to which the query row is added
__device__ __forceinline__ int64_t attn_part_row0(const AttnBase& p, const AttnWg& w) {
  const int64_t rows_all = (int64_t)gridDim.x / (p.qblocks * p.nsplit) * p.lq;  // batch * heads * lq
  return (int64_t)w.ksp * rows_all + ((int64_t)w.batch * p.heads + w.head) * p.lq;
}
// The end of a kernel on v_mfma_f32_16x16x32 accumulators: a wave owns the 64 query rows from wq0 as NQ = 4 blocks of 16, lane
// (i16 = lane & 15, g = lane >> 4) holds dims 16 db + 4 g .. + 3 of query i16 of each block in acc_o[c][db]; l[c] is that query's softmax
// denominator.
// K/V split: the partial result, un-normalised O (relative to m_run) as fp32, 16 bytes per lane and 16-dim block, and (m_run, l) per
// query row
template <int NQ>
__device__ __forceinline__ void attn_write_partial16(const AttnBase& p, const AttnWg& w, int wq0, const f32x4 (&acc_o)[NQ][4],
                                                     const float (&m_run)[NQ], const float (&l)[NQ], int i16, int g) {
  const int64_t row0 = attn_part_row0(p, w);
#pragma unroll
  for (int c = 0; c < NQ; ++c) {
    const int qrow = wq0 + 16 * c + i16;
    if (qrow < p.lq) {
      float* const po = p.part_o + (row0 + qrow) * 64;
#pragma unroll
      for (int db = 0; db < 4; ++db) *(f32x4*)(po + 16 * db + 4 * g) = acc_o[c][db];
      if (g == 0) {
        float* const pm = p.part_ml + (row0 + qrow) * 2;
        pm[0] = m_run[c];
        pm[1] = l[c];
      }
    }
  }
}
// otherwise: the normalised rows
template <int NQ>
__device__ __forceinline__ void attn_store_o16(char* smem, half_t* obase, int64_t o_sl, int wq0, int lq, const f32x4 (&acc_o)[NQ][4],
                                               const float (&l)[NQ], int lane, int wave, int i16, int g) {
  __syncthreads();  // every wave is done reading K/V tiles
  char* const ow = smem + wave * (64 * 128);
#pragma unroll
  for (int c = 0; c < NQ; ++c) {
    const float inv = 1.0f / l[c];
    const int row = 16 * c + i16;
#pragma unroll
    for (int db = 0; db < 4; ++db) attn_stage_o4(ow, row, 16 * db + 4 * g, acc_o[c][db], inv);
  }
  attn_store_rows<16 * NQ / 8>(ow, obase, o_sl, wq0, lq, lane);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// attention.hip: attn_combine_kernel over the K/V-split partials of any of the kernels (one partial layout)
int seva_attn_combine_launch(const float* part_o, const float* part_ml, int nsplit, void* out, int64_t o_sb0, int64_t o_sb1,
                             int64_t o_sl, int nb1, int heads, int lq, int64_t rows_all, hipStream_t s);

// the descriptor checks of every entry point; qo: the launch reads q and writes out (their strides count)
inline int attn_check_desc(const seva_attn_desc* d, const char* what, bool qo) {
  SEVA_REQUIRE(d != nullptr, "%s: null desc", what);
  SEVA_REQUIRE(d->lq > 0 && d->lk > 0 && d->heads > 0 && d->nb0 > 0 && d->nb1 > 0,
               "%s: empty problem lq=%d lk=%d heads=%d nb=%dx%d", what, d->lq, d->lk, d->heads, d->nb0, d->nb1);
  const int64_t qo_strides = qo ? d->q_sb0 | d->q_sb1 | d->q_sl | d->o_sb0 | d->o_sb1 | d->o_sl : 0;
  SEVA_REQUIRE((qo_strides | d->k_sb0 | d->k_sb1 | d->k_sl) % 8 == 0, "%s: strides must be multiples of 8 elements", what);
  return SEVA_OK;
}
// ... and of the buffers the launch touches
inline int attn_check_ptrs(const char* what, std::initializer_list<const void*> ptrs) {
  uintptr_t all = 0;
  for (const void* ptr : ptrs) {
    SEVA_REQUIRE(ptr != nullptr, "%s: null pointer", what);
    all |= (uintptr_t)ptr;
  }
  SEVA_REQUIRE(all % 16 == 0, "%s: pointers must be 16-byte aligned", what);
  return SEVA_OK;
}
inline int attn_check_grid(const char* what, int64_t nb) {
  SEVA_REQUIRE(nb > 0 && nb <= 0x7fffffff, "%s: bad grid %lld", what, (long long)nb);
  return SEVA_OK;
}
inline void attn_fill_base(AttnBase& a, const seva_attn_desc* d) {
  a.q = (const half_t*)d->q; a.k = (const half_t*)d->k; a.out = (half_t*)d->out;
  a.q_sb0 = d->q_sb0; a.q_sb1 = d->q_sb1; a.q_sl = d->q_sl;
  a.k_sb0 = d->k_sb0; a.k_sb1 = d->k_sb1; a.k_sl = d->k_sl;
  a.o_sb0 = d->o_sb0; a.o_sb1 = d->o_sb1; a.o_sl = d->o_sl;
  a.nb1 = d->nb1; a.heads = d->heads; a.lq = d->lq; a.lk = d->lk;
}
// K/V split into nsplit ranges of whole tiles: checks the workspace (seva_attn_desc.split_ws) and the grid of nb * nsplit workgroups
// and points the arguments at the partials; rows_all = batch * heads * lq
inline int attn_split_setup(AttnBase& a, const seva_attn_desc* d, const char* what, int nsplit, int64_t rows_all, int64_t nb) {
  static_assert(SEVA_ATTN_SPLIT_ROW_FLOATS == 64 + 2, "per split and query row: 64 floats of O in part_o, (m, l) in part_ml");
  const int64_t need = nsplit * rows_all * SEVA_ATTN_SPLIT_ROW_FLOATS * 4;
  SEVA_REQUIRE(d->split_ws_bytes >= need && (uintptr_t)d->split_ws % 16 == 0,
               "%s: split_ws too small (%lld bytes, need %lld) or misaligned", what, (long long)d->split_ws_bytes, (long long)need);
  SEVA_REQUIRE(nb * nsplit <= 0x7fffffff && rows_all * 8 / 256 + 1 <= 0x7fffffff, "%s: split grid too large", what);
  a.nsplit = nsplit;
  a.part_o = d->split_ws;
  a.part_ml = d->split_ws + (int64_t)nsplit * rows_all * 64;
  return SEVA_OK;
}
