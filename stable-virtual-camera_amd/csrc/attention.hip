// Flash-style scaled-dot-product attention for head dim 64 on gfx950 (MI355X), fp16 in/out.
//
// One wave owns 32 query rows.  Scores are computed TRANSPOSED, S^T = K * Q^T with
// v_mfma_f32_32x32x16_f16 (A = K rows from LDS, B = Q fragments kept in registers), so the query
// sits on the lane and a lane's 16 accumulator registers per 32-key block are 16 keys of ITS
// query: row max / row sum are register-local plus one exchange with lane^32.  The f32 scores,
// exponentiated and packed to fp16 in place, are directly the B operand of the second product
// O^T = V^T * P^T (accumulator-as-operand, k order permuted consistently on both operands); the
// V^T fragments come from the row-major V tile in LDS through ds_read_b64_tr_b16.  Online softmax
// in the log2 domain, fp32 throughout.
//
// K tile: 128-byte rows, 16-byte chunk c of row r stored at c ^ ((r>>1)&7)  (conflict-free b128 row reads)
// V tile: 128-byte rows, chunk c of row r stored at c ^ (((r>>1)&1)<<2)     (conflict-free tr reads)
//
// Regimes: per-frame / joint attention use 4 waves x 64-key tiles; the temporal
// regime (L = num_frames <= 32, batch = pixels) uses one wave per (pixel, head) with a 32-key
// tile and reads its tokens through the token stride, so no (b t) s c <-> (b s) t c transpose exists.
#include "attn_common.h"

#include <stdlib.h>

namespace {
// Two softmax probabilities -> one f16 pair, round to nearest even (v_cvt_pk_f16_f32, one instruction like the round-toward-zero pack
// it replaces).  A truncating pack cancels in O = sum(p v) / sum(p) to first order only: the key that sets the exponent reference has
// P = 1.0 exactly and loses nothing while every other key loses 2^-11 of its weight on average, so each row leaned towards its heaviest
// key and came out 3e-5 .. 6e-5 too large (tests/test_output_rounding_gpu.py::test_c_attention: `gain`).  A P above the f16 range now
// packs to inf, not 65504: its row sum is then inf, which every caller already routes to its rescale path (the sum / maximum tests).
typedef __fp16 p16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ p16x2_t pack_p(float e0, float e1) {
  return __builtin_bit_cast(p16x2_t, __builtin_convertvector(f32x2{e0, e1}, half2_t));
}

struct AttnArgs : AttnBase {};  // (its own type: the kernels' names carry it)

typedef short short8_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ half8_t tr_read_pair(const char* a0, const char* a1) {
  short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)a0);
  short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)a1);
  short8_t s = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(half8_t, s);
}

__device__ __forceinline__ int v_chunk_swz(int row, int chunk) { return chunk ^ (((row >> 1) & 1) << 2); }

// DBGK: the ablation instantiation reads p.dbg at run time; the production one has no such branches
// (they split the tile body into dozens of basic blocks and stop the scheduler interleaving
// LDS reads, MFMAs and the softmax VALU work across them).
// PRE: q already carries scale*log2(e) (folded into the producing GEMM's fp32 epilogue).  The score
// accumulators then START at -m_run (splat per key block: 16 moves instead of 32 v_fma), so
// S^T = K Q^T comes out of the MFMA already in exp2's argument form.
// max over the two half-waves (lanes l and l ^ 32) in every lane.  v_permlane32_swap exchanges the upper half of its first
// operand with the lower half of its second: (a, b) = (v, v) -> a = {v.lo, v.lo}, b = {v.hi, v.hi}.  Inline asm: the
// builtin of this toolchain returns element 0 of its result pair for both elements (checked on a probe kernel); the s_nop
// covers the VALU-write -> permlane-read wait states the compiler would insert for the builtin.
__device__ __forceinline__ float half_wave_max(float v) {
  float a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return fmaxf(a, b);
}

// NBUF: buffers of the K/V ring.  3 is the ring.  1 is the short-sequence form (lk <= KT, the host's rule): the only tile goes to the
// only buffer, nothing is prefetched (nt == 1: attn_ring_start issues tile 0 alone and attn_ring_prefetch never fires), and the
// workgroup holds 2 * KT * 128 bytes of LDS instead of three times that.
template <int NW, int KT, bool USE_TR, bool DBGK, bool PRE, int NBUF = 3>
__global__ __launch_bounds__(NW * 64, 3) void attn_kernel(AttnArgs p) {
  constexpr int KB = KT / 32;               // 32-key blocks per tile
  const int dbg = DBGK ? p.dbg : 0;
  static_assert(NBUF == 3 || NBUF == 1, "the three-buffer ring, or one buffer for a single tile");
  static_assert(NBUF * 2 * KT * 128 >= NW * 32 * 128, "the epilogue stages NW images of 32 rows in the K/V buffers");

  __shared__ __attribute__((aligned(16))) char smem[NBUF * 2 * KT * 128];  // the K/V ring: [buf][K tile | V tile]
  constexpr int BUF_BYTES = 2 * KT * 128;
  typedef AttnRing<KT, NW, BUF_BYTES, v_chunk_swz> Ring;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int qi = lane & 31, hh = lane >> 5;

  AttnWg w;
  attn_decode<false>(p, KT, w);
  const int qb = w.qb;
  const half_t* const qbase = attn_q_base(p, w);
  const half_t* const kbase = attn_kv_base(p, w, p.k);
  const half_t* const vbase = attn_kv_base(p, w, p.v);
  half_t* const obase = attn_o_base(p, w);

  const int qrow = qb * (32 * NW) + wave * 32 + qi;
  const int qrow_c = qrow < p.lq ? qrow : p.lq - 1;

  half8_t qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
    qf[s] = *(const half8_t*)(qbase + (int64_t)qrow_c * p.q_sl + 16 * s + 8 * hh);

  f32x16 acc_o[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_o[d][r] = 0.f;
  // m_run is the exponent reference in the log2 domain (scaled scores); it may lag the true running
  // max by up to RESCALE_THR (deferred rescale), so probabilities are bounded by 2^RESCALE_THR.
  constexpr float RESCALE_THR = 8.0f;
  float m_run = PRE ? 0.f : -1e30f, l_run = 0.f;
  // PRE: -m_run held as a 16-register block = the C operand of the first score MFMA of every key block (rebuilt only when
  // m_run moves, i.e. in the rare rescale branch, instead of 15 v_mov per tile)
  f32x16 neg_m[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) neg_m[0][r] = neg_m[1][r] = 0.f;
  const float c = p.scale_log2;

  const int nt = (p.lk + KT - 1) / KT;
  Ring ring(kbase, vbase, p.k_sl, p.lk, smem, lane, wave);

  const int g16 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3;

  // one K/V tile (the ring driver: attn_common.h)
  auto tile = [&](int buf, auto masked_c, int kt) {
    constexpr bool MASKED = decltype(masked_c)::value;
    const char* const lds_k = smem + buf * BUF_BYTES;
    const char* const lds_v = lds_k + KT * 128;
    const bool more2 = attn_ring_prefetch(kt, nt, buf, !(dbg & 1), ring);

    // ---- S^T = K Q^T ----
    f32x16 sc[KB];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const int krow = 32 * kb + qi;
      if (!(dbg & 8)) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const half8_t kf =
              *(const half8_t*)(lds_k + krow * 128 + (k_chunk_swz(krow, 2 * s + hh) << 4));
          if (s == 0) {
            f32x16 c0;
            if (PRE) {
              c0 = neg_m[kb & 1];
            } else {
#pragma unroll
              for (int r = 0; r < 16; ++r) c0[r] = 0.f;
            }
            sc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], c0, 0, 0, 0);
          } else {
            sc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], sc[kb], 0, 0, 0);
          }
        }
      } else {
        asm volatile("" : "=v"(sc[kb]));
      }
    }
    __builtin_amdgcn_s_setprio(0);
    if (MASKED) {  // keys >= lk exist only in the last tile
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kt * KT + 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * hh;
          if (key >= p.lk) sc[kb][r] = -1e30f;
        }
    }
    // ---- online softmax, log2 domain, deferred rescale ----
    float mx = -1e30f;
    if (!(dbg & 2)) {
      // one max chain per key block (independent: half the dependent-issue depth), then the other half-wave's maximum of the
      // same query by v_permlane32_swap (a VALU op; ds_bpermute costs an LDS round trip and an lgkmcnt(0) per tile)
      float mk[KB];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        mk[kb] = sc[kb][0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mk[kb] = fmaxf(mk[kb], sc[kb][r]);
      }
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) mx = fmaxf(mx, mk[kb]);
      mx = half_wave_max(mx);
    }
    if (PRE) {
      // scores are already relative to m_run: rescale when a row maximum exceeds the threshold, and
      // unconditionally on the first tile (m_run starts at 0; nothing accumulated yet, so alpha = 1)
      const bool first = kt == 0;
      if (!(dbg & 2) && (first || __any(mx > RESCALE_THR))) {  // wave-uniform
        const float delta = first ? mx : fmaxf(mx, 0.f);
        const float alpha = first ? 1.0f : __builtin_amdgcn_exp2f(-delta);
        m_run += delta;
#pragma unroll
        for (int r = 0; r < 16; ++r) neg_m[0][r] = neg_m[1][r] = -m_run;
        asm volatile("" : "+v"(neg_m[0]), "+v"(neg_m[1]));  // two distinct blocks (not one value the compiler may merge)
        l_run *= alpha;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc_o[d][r] *= alpha;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) sc[kb][r] -= delta;
      }
    } else {
    const float mxs = mx * c;  // c > 0
    if (!(dbg & 2) && __any(mxs > m_run + RESCALE_THR)) {  // wave-uniform
      const float m_new = fmaxf(m_run, mxs);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[d][r] *= alpha;
    }
    }
    // P = exp2(S*c - m) packed to fp16 pairs (pack_p: round to nearest even); the row sum is taken from the
    // ROUNDED values (v_dot2_f32_f16 with ones) so numerator (P*V) and normaliser see identical
    // probabilities and the rounding cancels in O = sum(p v) / sum(p).
    typedef __fp16 fp16x2_t __attribute__((ext_vector_type(2)));
    const fp16x2_t ones2 = {(__fp16)1.0f, (__fp16)1.0f};
    float lsum4[4] = {0.f, 0.f, 0.f, 0.f};  // four independent dot2 chains
    half8_t pf[KB][2];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        fp16x2_t pk[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float e0, e1;
          if (!(dbg & 2)) {
            if (PRE) {
              e0 = __builtin_amdgcn_exp2f(sc[kb][8 * s2 + 2 * j]);
              e1 = __builtin_amdgcn_exp2f(sc[kb][8 * s2 + 2 * j + 1]);
            } else {
              e0 = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kb][8 * s2 + 2 * j], c, -m_run));
              e1 = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kb][8 * s2 + 2 * j + 1], c, -m_run));
            }
          } else {
            e0 = sc[kb][8 * s2 + 2 * j];
            e1 = sc[kb][8 * s2 + 2 * j + 1];
          }
          pk[j] = pack_p(e0, e1);
          if (!(dbg & 2)) lsum4[j] = __builtin_amdgcn_fdot2(pk[j], ones2, lsum4[j], false);
        }
        pf[kb][s2] = __builtin_bit_cast(half8_t, pk);
      }
    l_run += (lsum4[0] + lsum4[1]) + (lsum4[2] + lsum4[3]);

    // ---- O^T += V^T P^T ----
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int db = 0; db < 2; ++db) {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const int r0 = 32 * kb + 16 * s2 + 4 * hh;
          half8_t vf;
          if (USE_TR) {
            const int colbyte = (32 * db + 16 * (g16 & 1) + 4 * p4) * 2;
            const int ch = colbyte >> 4, within = colbyte & 15;
            const int ra = r0 + q4, rb = r0 + 8 + q4;
            vf = tr_read_pair(lds_v + ra * 128 + (v_chunk_swz(ra, ch) << 4) + within,
                              lds_v + rb * 128 + (v_chunk_swz(rb, ch) << 4) + within);
          } else {
            const int d = 32 * db + qi;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int row = r0 + (j & 3) + 8 * (j >> 2);
              vf[j] = *(const half_t*)(lds_v + row * 128 + (v_chunk_swz(row, d >> 3) << 4) + (d & 7) * 2);
            }
          }
          if (!(dbg & 4)) acc_o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[kb][s2], acc_o[db], 0, 0, 0);
          else asm volatile("" ::"v"(vf), "v"(pf[kb][s2]));
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    attn_ring_arrive<Ring::G>(more2);
  };
  attn_ring_start<Ring::G>(nt, ring, qf);
  const int nfull = p.lk / KT;  // tiles that need no mask (the ragged tail tile, if any, is the last one)
  int buf = 0;                  // buffer index == tile % 3
  for (int kt = 0; kt < nfull; ++kt) {
    tile(buf, std::false_type{}, kt);
    buf = buf == 2 ? 0 : buf + 1;
  }
  if (nfull < nt) tile(buf, std::true_type{}, nfull);

  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / l_tot;
  __syncthreads();  // every wave is done reading K/V tiles
  char* const ow = smem + wave * (32 * 128);
  attn_stage_o32(ow, qi, hh, acc_o, inv);
  attn_store_rows<4>(ow, obase, p.o_sl, qb * (32 * NW) + wave * 32, p.lq, lane);
}

// ---------------------------------------------------------------------------------------------
// Two-query-block variant for long sequences (engine path: pre-scaled q, tr-reads): a wave owns 64 query rows as two 32-row
// blocks A and B (2 waves per SIMD) and every K fragment and V^T fragment it reads from LDS feeds BOTH blocks' MFMAs:
//   scores(A, B) | softmax(A) | softmax(B) | PV(A, B)
// Per query that is half the LDS fragment reads, half the K/V LDS-DMA bytes and instructions (a workgroup's tile serves 256
// queries) and half the per-tile bookkeeping of attn_kernel -- the components whose costs ADD UP there (ablations of
// the pipelined kernel).  Same LDS ring, operand layouts, online-softmax arithmetic and rounding as
// attn_kernel<4, 64, true, false, true> (ring and driver: attn_common.h); half-wave maximum by v_permlane32_swap (as there).
template <int KT, bool SPLIT = false>
__global__ __launch_bounds__(256, 2) void attn2_kernel(AttnArgs p) {
  constexpr int NW = 4, QB = 2, KB = KT / 32;
  // SPLIT: this workgroup walks only the K/V tiles [ksp * tps, (ksp + 1) * tps) of its (batch, head) and writes a partial result.
  // Workgroups of one (batch, head, split) are adjacent in the launch order (they stream the same K/V range through one L2).
  __shared__ __attribute__((aligned(16))) char smem[3 * 2 * KT * 128];
  constexpr int BUF_BYTES = 2 * KT * 128;
  typedef AttnRing<KT, NW, BUF_BYTES, v_chunk_swz> Ring;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int qi = lane & 31, hh = lane >> 5;

  AttnWg w;
  attn_decode<SPLIT>(p, KT, w);
  const int qb = w.qb, lk = w.lk;
  const half_t* const qbase = attn_q_base(p, w);
  const half_t* const kbase = attn_kv_base(p, w, p.k);
  const half_t* const vbase = attn_kv_base(p, w, p.v);
  half_t* const obase = attn_o_base(p, w);

  half8_t qf[QB][4];
#pragma unroll
  for (int c = 0; c < QB; ++c) {
    const int qrow = qb * (32 * QB * NW) + wave * (32 * QB) + 32 * c + qi;
    const int qrow_c = qrow < p.lq ? qrow : p.lq - 1;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      qf[c][s] = *(const half8_t*)(qbase + (int64_t)qrow_c * p.q_sl + 16 * s + 8 * hh);
  }

  // a wave whose 64 query rows all lie past lq (ragged last query block: 5184 = 20.25 x 256) keeps feeding the K/V ring and
  // meeting the barriers but computes nothing: its MFMA / VALU / LDS-read slots go to the other workgroup on the CU
  const bool active = __builtin_amdgcn_readfirstlane(qb * (32 * QB * NW) + wave * (32 * QB)) < p.lq;
  f32x16 acc_o[QB][2];
  float m_run[QB], l_run[QB];
  // -m_run as a 16-register block per query block: the C operand of the first score MFMA of every key block (as in attn_kernel),
  // rebuilt only in the rare rescale branch: 64 v_mov per tile fewer in a loop whose VALU work, not its MFMA work, sets the pace
  f32x16 neg_m[QB];
#pragma unroll
  for (int c = 0; c < QB; ++c) {
    m_run[c] = 0.f;
    l_run[c] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) neg_m[c][r] = 0.f;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc_o[c][d][r] = 0.f;
  }
  constexpr float P_SUM_BOUND = 16384.0f;  // a lane's partial row sum at or above 2^14: look at the maximum, rescale (see the tile body)

  const int nt = (lk + KT - 1) / KT;
  Ring ring(kbase, vbase, p.k_sl, lk, smem, lane, wave);
  const int g16 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3;
  typedef __fp16 fp16x2_t __attribute__((ext_vector_type(2)));
  const fp16x2_t ones2 = {(__fp16)1.0f, (__fp16)1.0f};

  auto tile = [&](int buf, auto masked_c, int kt) {
    constexpr bool MASKED = decltype(masked_c)::value;
    const char* const lds_k = smem + buf * BUF_BYTES;
    const char* const lds_v = lds_k + KT * 128;
    const bool more2 = attn_ring_prefetch(kt, nt, buf, true, ring);

    if (active) {
    // ---- S^T = K Q^T for both query blocks off ONE K fragment; accumulators start at -m_run (q carries scale*log2e) ----
    f32x16 sc[QB][KB];
    __builtin_amdgcn_s_setprio(1);
    if constexpr (!SPLIT) {
      // every K fragment of the tile is ISSUED before the first score MFMA (hipcc otherwise reads one pair ahead and waits for it in front
      // of every two MFMAs).  Measured, same box (profiles/r04_kattn_frags_first.log): per-frame attention at 72x72 1834 -> 1788 us; the K/V-split
      // instantiation spills 7 registers with it and keeps hipcc's order; the same for the V^T fragments of the P V phase loses 1 - 3 %
      half8_t kfa[KB][4];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const int krow = 32 * kb + qi;
#pragma unroll
        for (int s = 0; s < 4; ++s) kfa[kb][s] = *(const half8_t*)(lds_k + krow * 128 + (k_chunk_swz(krow, 2 * s + hh) << 4));
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int c = 0; c < QB; ++c)
            sc[c][kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfa[kb][s], qf[c][s], s == 0 ? neg_m[c] : sc[c][kb], 0, 0, 0);
    } else {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const int krow = 32 * kb + qi;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const half8_t kf = *(const half8_t*)(lds_k + krow * 128 + (k_chunk_swz(krow, 2 * s + hh) << 4));
#pragma unroll
        for (int c = 0; c < QB; ++c) {
          if (s == 0) {
            sc[c][kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[c][s], neg_m[c], 0, 0, 0);
          } else {
            sc[c][kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[c][s], sc[c][kb], 0, 0, 0);
          }
        }
      }
    }
    }
    __builtin_amdgcn_s_setprio(0);
    // ---- online softmax per query block: mask, running maximum, rare rescale; exp2 / pack / row sums ----
    half8_t pf[QB][KB][2];
#pragma unroll
    for (int c = 0; c < QB; ++c) {
      if (MASKED) {
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = kt * KT + 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (key >= lk) sc[c][kb][r] = -1e30f;
          }
      }
      // exp2 / pack / row sums FIRST, straight off the scores relative to m_run; the running maximum is looked at only when a
      // partial row sum says a probability may have left the safe range (any P >= 2^14 makes its lane's sum >= 2^14; f16 holds
      // 2^16 - 32 and a larger P packs to inf, which makes the sum inf: the test below sees that too), and on the first tile
      // (m_run = 0 there: the true maximum protects the small probabilities from underflow).  The 21 v_max3 + the half-wave
      // exchange per query block leave the steady-state loop.
      float ls[4];
      const auto exp_pack = [&]() {
        ls[0] = ls[1] = ls[2] = ls[3] = 0.f;  // four partial sums: short dependent dot2 chains
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            fp16x2_t pk[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float e0 = __builtin_amdgcn_exp2f(sc[c][kb][8 * s2 + 2 * j]);
              const float e1 = __builtin_amdgcn_exp2f(sc[c][kb][8 * s2 + 2 * j + 1]);
              pk[j] = pack_p(e0, e1);
              ls[j] = __builtin_amdgcn_fdot2(pk[j], ones2, ls[j], false);
            }
            pf[c][kb][s2] = __builtin_bit_cast(half8_t, pk);
          }
        return (ls[0] + ls[1]) + (ls[2] + ls[3]);
      };
      float tot = exp_pack();
      const bool first = kt == 0;
      if (__builtin_expect(first || __any(!(tot < P_SUM_BOUND)), 0)) {  // wave-uniform, rare (NaN / inf sums land here too)
        float mk[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
          mk[kb] = sc[c][kb][0];
#pragma unroll
          for (int r = 1; r < 16; ++r) mk[kb] = fmaxf(mk[kb], sc[c][kb][r]);
        }
        float mx = mk[0];
#pragma unroll
        for (int kb = 1; kb < KB; ++kb) mx = fmaxf(mx, mk[kb]);
        mx = half_wave_max(mx);
        const float delta = first ? mx : fmaxf(mx, 0.f);
        const float alpha = first ? 1.0f : __builtin_amdgcn_exp2f(-delta);
        m_run[c] += delta;
        l_run[c] *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) neg_m[c][r] = -m_run[c];
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc_o[c][d][r] *= alpha;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) sc[c][kb][r] -= delta;
        tot = exp_pack();
      }
      l_run[c] += tot;
    }
    // ---- O^T += V^T P^T for both query blocks off ONE V^T fragment ----
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const int r0 = 32 * kb + 16 * s2 + 4 * hh;
          const int colbyte = (32 * db + 16 * (g16 & 1) + 4 * p4) * 2;
          const int ch = colbyte >> 4, within = colbyte & 15;
          const int ra = r0 + q4, rb = r0 + 8 + q4;
          const half8_t vf = tr_read_pair(lds_v + ra * 128 + (v_chunk_swz(ra, ch) << 4) + within,
                                          lds_v + rb * 128 + (v_chunk_swz(rb, ch) << 4) + within);
#pragma unroll
          for (int c = 0; c < QB; ++c)
            acc_o[c][db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[c][kb][s2], acc_o[c][db], 0, 0, 0);
        }
    __builtin_amdgcn_s_setprio(0);
    }  // active
    attn_ring_arrive<Ring::G>(more2);
  };
  attn_ring_start<Ring::G>(nt, ring, qf);
  const int nfull = lk / KT;
  int buf = 0;
  for (int kt = 0; kt < nfull; ++kt) {
    tile(buf, std::false_type{}, kt);
    buf = buf == 2 ? 0 : buf + 1;
  }
  if (nfull < nt) tile(buf, std::true_type{}, nfull);

  if constexpr (SPLIT) {
    // partial result: un-normalised O (relative to m_run) as fp32, 16 bytes per lane and (db, t), and (m_run, l) per query row
    const int64_t row0 = attn_part_row0(p, w);
#pragma unroll
    for (int c = 0; c < QB; ++c) {
      const int qrow = qb * (32 * QB * NW) + wave * (32 * QB) + 32 * c + qi;
      const float l_tot = l_run[c] + __shfl_xor(l_run[c], 32, 64);
      if (qrow < p.lq) {
        float* const po = p.part_o + (row0 + qrow) * 64;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            *(f32x4*)(po + 32 * db + 8 * t + 4 * hh) =
                f32x4{acc_o[c][db][4 * t], acc_o[c][db][4 * t + 1], acc_o[c][db][4 * t + 2], acc_o[c][db][4 * t + 3]};
        if (hh == 0) {
          float* const pm = p.part_ml + (row0 + qrow) * 2;
          pm[0] = m_run[c];
          pm[1] = l_tot;
        }
      }
    }
    return;
  }
  __syncthreads();  // every wave is done reading K/V tiles
  char* const ow = smem + wave * QB * (32 * 128);  // the QB blocks' images are consecutive: 64 rows
#pragma unroll
  for (int c = 0; c < QB; ++c) {
    const float l_tot = l_run[c] + __shfl_xor(l_run[c], 32, 64);
    attn_stage_o32(ow + c * (32 * 128), qi, hh, acc_o[c], 1.0f / l_tot);
  }
  attn_store_rows<4 * QB>(ow, obase, p.o_sl, qb * (32 * QB * NW) + wave * (32 * QB), p.lq, lane);
}

// ---------------------------------------------------------------------------------------------
// attn2_kernel's two-block scheme on v_mfma_f32_16x16x32_f16: a wave owns 64 query rows as FOUR 16-row blocks and every K fragment
// and V^T fragment it reads from LDS feeds all four blocks' MFMAs.  Why the other MFMA shape: the chip holds its clock down under
// matrix load, and lower for v_mfma_f32_32x32x16 than for 16x16x32 -- the same FLOP took 653 ns against 553 ns in bare loops on random
// data (1.63 against 1.97 GHz; tools/micro/pingpong_probe.hip, profiles/r04_pingpong_probe.log; MI355X guide, DVFS item 7), and
// in this kernel MFMA time and VALU time ADD (same probe: neither SIMD partners nor one wave's own stream overlap them).
// Per 64 x 64 tile and wave: 8 K fragments, 8 V^T fragment pairs, 64 exp2, 32 packs as attn2_kernel; 72 MFMAs of 16 cycles instead of 32
// of 32; the -m_run C-operand block is 4 registers per query block instead of 16.
// The softmax row sums are 8 of the 72 MFMAs, not VALU work (attn2_kernel: 32 dot2 in four chains per block, their adds, two shuffles
// per block after the loop): P^T, rounded to f16, is the B operand of the P.V product already, and against an A fragment of ONES that
// product is sum_keys P of query i16 in every output row -- the full 64-key sum, in all four lanes of the query.  The steady-state
// tile is about 115 VALU instructions beside 72 MFMAs (before: 160 beside 64), and since matrix and vector time ADD on this chip (see
// above) the 128 matrix cycles buy more vector cycles than they cost (profiles/attention_rowsum.log).
// ONE rare branch per tile: exp2 / pack / sums of all four blocks, then one wave-uniform test of the four sums against the bound.  Inside
// it the decision stays per query block but as a select (delta = 0 leaves a block bit for bit as it was), and the scores come from the
// K tile again: kept in registers for the branch, the 64 score registers no longer die into P and the kernel spills.  Tile 0, which
// always sets the exponent reference, is its own instantiation of the body (FIRST) in front of the loop.
//   S^T block (16 keys x 16 queries) = K(16 x 32 d) Q^T: lane (i16 = lane & 15, g = lane >> 4) holds keys 4g .. 4g+3 of query i16
//   P^T as B operand of O^T(16 d x 16 queries) += V^T(16 d x 32 keys) P^T: the 32 keys of a step are two 16-key blocks in the order
//   kappa = 8g + r <-> key 4g + r of block 2j, kappa = 8g + 4 + r <-> key 4g + r of block 2j + 1: a lane's B fragment is its own
//   registers of the two blocks, and the V^T fragment is two ds_read_b64_tr_b16 of rows 32j + 4g .. +3 and 32j + 16 + 4g .. +3.
// K tile: attn_kernel's swizzle (conflict-free for these b128 reads too); V tile: chunk c of row r at c ^ (((r >> 1) & 3) << 1).
// Not bitwise equal to the 32x32x16 kernels (the MFMA shapes sum their k products in different orders): tested against fp64.
__device__ __forceinline__ int v16_chunk_swz(int row, int chunk) { return chunk ^ (((row >> 1) & 3) << 1); }

template <int KT, bool SPLIT = false>
__global__ __launch_bounds__(256, 2) void attn16_kernel(AttnArgs p) {
  constexpr int NW = 4, NQ = 4, NKB = KT / 16, NJ = KT / 32;
  __shared__ __attribute__((aligned(16))) char smem[3 * 2 * KT * 128];
  constexpr int BUF_BYTES = 2 * KT * 128;
  typedef AttnRing<KT, NW, BUF_BYTES, v16_chunk_swz> Ring;
  static_assert(3 * BUF_BYTES >= NW * 64 * 128, "the output staging re-uses the ring");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;

  AttnWg w;
  attn_decode<SPLIT>(p, KT, w);
  const int qb = w.qb, lk = w.lk;
  const half_t* const qbase = attn_q_base(p, w);
  const half_t* const kbase = attn_kv_base(p, w, p.k);
  const half_t* const vbase = attn_kv_base(p, w, p.v);
  half_t* const obase = attn_o_base(p, w);

  const int wq0 = qb * (64 * NW) + wave * 64;  // first query row of this wave
  half8_t qf[NQ][2];
#pragma unroll
  for (int c = 0; c < NQ; ++c) {
    const int qrow = wq0 + 16 * c + i16;
    const int qrow_c = qrow < p.lq ? qrow : p.lq - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[c][ks] = *(const half8_t*)(qbase + (int64_t)qrow_c * p.q_sl + 32 * ks + 8 * g);
  }
  // a wave whose 64 query rows all lie past lq keeps feeding the K/V ring and meeting the barriers but computes nothing
  const bool active = __builtin_amdgcn_readfirstlane(wq0) < p.lq;
  f32x4 acc_o[NQ][4];  // [query block][16-dim block]: dims 4g .. 4g+3 of query i16
  float m_run[NQ], l_run[NQ];
  f32x4 neg_m[NQ];     // -m_run: the C operand of the first score MFMA of every key block
#pragma unroll
  for (int c = 0; c < NQ; ++c) {
    m_run[c] = 0.f;
    l_run[c] = 0.f;
    neg_m[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < 4; ++d) acc_o[c][d] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // a query's 64-key row sum of one tile at or above 2^14: look at the maximum, rescale.  Still 2^14, attn2_kernel's bound on a lane's
  // 16-key partial sum: the bound keeps P inside f16 with margin, and the full row's sum crosses it no later than any of its parts did.
  constexpr float P_SUM_BOUND = 16384.0f;

  const int nt = (lk + KT - 1) / KT;
  Ring ring(kbase, vbase, p.k_sl, lk, smem, lane, wave);
  const int q4 = i16 >> 2, p4 = i16 & 3;
  typedef __fp16 fp16x2_t __attribute__((ext_vector_type(2)));
  half8_t ones8;  // the A fragment of the row-sum MFMAs
#pragma unroll
  for (int r = 0; r < 8; ++r) ones8[r] = (half_t)1.0f;

  // FIRST: tile 0 of this workgroup's keys, which always sets the exponent reference; the steady-state tile has no such case
  auto tile = [&](int buf, auto masked_c, auto first_c, int kt) {
    constexpr bool MASKED = decltype(masked_c)::value;
    constexpr bool FIRST = decltype(first_c)::value;
    const char* const lds_k = smem + buf * BUF_BYTES;
    const char* const lds_v = lds_k + KT * 128;
    const bool more2 = attn_ring_prefetch(kt, nt, buf, true, ring);

    if (active) {
      // ---- S^T = K Q^T for the four query blocks off ONE K fragment; accumulators start at -m_run (q carries scale*log2e) ----
      f32x4 sc[NQ][NKB];
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        const int krow = 16 * kb + i16;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const half8_t kf = *(const half8_t*)(lds_k + krow * 128 + (k_chunk_swz(krow, 4 * ks + g) << 4));
#pragma unroll
          for (int c = 0; c < NQ; ++c)
            sc[c][kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[c][ks], ks == 0 ? neg_m[c] : sc[c][kb], 0, 0, 0);
        }
      }
      // ---- online softmax per query block: exp2 / pack / row sums first, the maximum only on the rare path ----
      half8_t pf[NQ][NJ];
      const auto mask_tail = [&](f32x4 (&s)[NKB]) {
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (kt * KT + 16 * kb + 4 * g + r >= lk) s[kb][r] = -1e30f;
      };
      // P of query block c, rounded to f16, and its row sums ON THE MATRIX PIPE: with an A fragment of ones, the product that adds
      // V^T P^T gives sum_keys P of query i16 in every row of its output block, so every lane holds in element 0 the 64-key sum of
      // ITS query, taken from the rounded P (the quotient O / l loses nothing to the rounding: tests/test_output_rounding_gpu.py)
      const auto exp_pack = [&](int c, const f32x4 (&s)[NKB]) {
        f32x4 tl = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          fp16x2_t pk[4];
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              const float e0 = __builtin_amdgcn_exp2f(s[2 * j + h][2 * e]);
              const float e1 = __builtin_amdgcn_exp2f(s[2 * j + h][2 * e + 1]);
              pk[2 * h + e] = pack_p(e0, e1);
            }
          pf[c][j] = __builtin_bit_cast(half8_t, pk);
          tl = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones8, pf[c][j], tl, 0, 0, 0);
        }
        return tl[0];
      };
      // the rare path of one query block, on its (masked) scores s: move the exponent reference to the block maximum, P and sums again
      const auto new_reference = [&](int c, f32x4 (&s)[NKB], bool need) {
        float mx = s[0][0];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kb][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));  // the four lanes of a query: lane groups g = 0 .. 3
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float delta = FIRST ? mx : need ? fmaxf(mx, 0.f) : 0.f;
        m_run[c] += delta;
#pragma unroll
        for (int r = 0; r < 4; ++r) neg_m[c][r] = -m_run[c];
        if (!FIRST) {  // (tile 0: l_run and acc_o are zero)
          const float alpha = __builtin_amdgcn_exp2f(-delta);
          l_run[c] *= alpha;
#pragma unroll
          for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc_o[c][d][r] *= alpha;
        }
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[kb][r] -= delta;
        return exp_pack(c, s);
      };
      float tot[NQ];
      if (FIRST) {
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
          if (MASKED) mask_tail(sc[c]);
          tot[c] = new_reference(c, sc[c], true);
        }
      } else {
        // all four blocks first (block c's row-sum MFMAs finish under block c + 1's exponentials), then ONE wave-uniform test.  The
        // scores die into P block by block, as they always did: kept for the rare path they would cost 64 registers more than the two
        // workgroups per CU leave.
        bool over = false;
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
          if (MASKED) mask_tail(sc[c]);
          tot[c] = exp_pack(c, sc[c]);
          if (c > 0) over |= !(tot[c - 1] < P_SUM_BOUND);  // (one block behind: its MFMAs have finished)
          __builtin_amdgcn_sched_barrier(0);  // block by block: mixed freely, the four blocks' temporaries do not fit in 256 registers
        }
        over |= !(tot[NQ - 1] < P_SUM_BOUND);
        if (__builtin_expect(__any(over), 0)) {  // wave-uniform, rare (NaN / inf sums land here too)
          // The decision stays per query block and wave-uniform, but as a select, not a branch (four more branches with the accumulators
          // live across them, and hipcc spills the accumulators in EVERY tile): a block whose own sums were below the bound gets
          // delta = 0, alpha = 1, which leaves its reference, accumulators, P and sums bit for bit as they were.
#pragma unroll
          for (int c = 0; c < NQ; ++c) {
            const bool need = __any(!(tot[c] < P_SUM_BOUND));
            // the block's scores again, from the K tile (still in LDS) and the old reference: the same MFMAs, the same bits
            f32x4 s1[NKB];
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
              const int krow = 16 * kb + i16;
#pragma unroll
              for (int ks = 0; ks < 2; ++ks) {
                const half8_t kf = *(const half8_t*)(lds_k + krow * 128 + (k_chunk_swz(krow, 4 * ks + g) << 4));
                s1[kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[c][ks], ks == 0 ? neg_m[c] : s1[kb], 0, 0, 0);
              }
            }
            if (MASKED) mask_tail(s1);
            tot[c] = new_reference(c, s1, need);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < NQ; ++c) l_run[c] += tot[c];
      // ---- O^T += V^T P^T for the four query blocks off ONE V^T fragment ----
      // all eight V^T fragments are ISSUED before the first MFMA (the scores' registers are free by now): read one pair ahead, as hipcc
      // orders them, every group of eight MFMAs waits for its LDS round trip.  Same-box A/B (profiles/r04_kattn16.log): per-frame
      // attention at 72x72 1462 -> 1409 us, joint at 36x36 3429 -> 3401; the same for the K fragments of the score phase changes nothing.
      half8_t vfa[4][NJ];
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int ra = 32 * j + 4 * g + q4, rb = ra + 16;
          const int colbyte = (16 * db + 4 * p4) * 2;
          const int ch = colbyte >> 4, within = colbyte & 15;
          vfa[db][j] = tr_read_pair(lds_v + ra * 128 + (v16_chunk_swz(ra, ch) << 4) + within,
                                    lds_v + rb * 128 + (v16_chunk_swz(rb, ch) << 4) + within);
        }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int c = 0; c < NQ; ++c) acc_o[c][db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vfa[db][j], pf[c][j], acc_o[c][db], 0, 0, 0);
    }  // active
    attn_ring_arrive<Ring::G>(more2);
  };
  attn_ring_start<Ring::G>(nt, ring, qf);
  const int nfull = lk / KT;
  // tile 0 (buffer 0) on its own: the only one that always sets the exponent reference.  nt == 1 with a ragged tile: masked AND first
  if (nfull > 0) tile(0, std::false_type{}, std::true_type{}, 0);
  else tile(0, std::true_type{}, std::true_type{}, 0);
  int buf = 1;
  for (int kt = 1; kt < nfull; ++kt) {
    tile(buf, std::false_type{}, std::false_type{}, kt);
    buf = buf == 2 ? 0 : buf + 1;
  }
  if (nfull > 0 && nfull < nt) tile(buf, std::true_type{}, std::false_type{}, nfull);

  // every lane of a query holds the full sums: nothing to exchange
  float l_tot[NQ];
#pragma unroll
  for (int c = 0; c < NQ; ++c) l_tot[c] = l_run[c];
  if constexpr (SPLIT) {
    attn_write_partial16(p, w, wq0, acc_o, m_run, l_tot, i16, g);
    return;
  }
  attn_store_o16(smem, obase, p.o_sl, wq0, p.lq, acc_o, l_tot, lane, wave, i16, g);
}

// Combine of the K/V-split partials: out = sum_i 2^(m_i - m*) O_i / sum_i 2^(m_i - m*) l_i, one thread per (row, 8 columns).
// Fixed order over the splits, exp2 of exact differences: deterministic, and (the split being a function of the sequence
// lengths only) independent of what else is in the batch.
__global__ __launch_bounds__(256) void attn_combine_kernel(AttnArgs p, int64_t rows_all) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows_all * 8) return;
  const int64_t row = i >> 3;
  const int ch = (int)(i & 7);
  float m[4], l[4], mx = -3.0e38f;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s < p.nsplit) {
      const float* pm = p.part_ml + ((int64_t)s * rows_all + row) * 2;
      m[s] = pm[0];
      l[s] = pm[1];
      mx = fmaxf(mx, m[s]);
    }
  float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, lt = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s < p.nsplit) {
      const float w = __builtin_amdgcn_exp2f(m[s] - mx);
      lt += w * l[s];
      const float* po = p.part_o + ((int64_t)s * rows_all + row) * 64 + 8 * ch;
      const f32x4 a = first_read(*(const f32x4*)po), b = first_read(*(const f32x4*)(po + 4));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        o[r] += w * a[r];
        o[4 + r] += w * b[r];
      }
    }
  const float inv = 1.0f / lt;
  half8_t h;
#pragma unroll
  for (int r = 0; r < 8; ++r) h[r] = (half_t)(o[r] * inv);
  // row = (batch * heads + head) * lq + q
  const int64_t q = row % p.lq, bh = row / p.lq;
  const int head = (int)(bh % p.heads);
  const int64_t batch = bh / p.heads;
  const int64_t b0 = batch / p.nb1, b1 = batch - b0 * p.nb1;
  *(half8_t*)(p.out + b0 * p.o_sb0 + b1 * p.o_sb1 + head * 64 + q * p.o_sl + 8 * ch) = h;
}


template <int NW, int KT, int NBUF = 3>
int launch(const AttnArgs& a, int64_t batch, hipStream_t s, bool use_tr, bool pre) {
  AttnArgs args = a;
  args.qblocks = (a.lq + 32 * NW - 1) / (32 * NW);
  SEVA_REQUIRE(NBUF == 3 || a.lk <= KT, "attention: the one-buffer kernel takes one K/V tile (lk=%d > %d)", a.lk, KT);
  const int64_t nb = batch * a.heads * args.qblocks;
  if (int rc = attn_check_grid("attention", nb)) return rc;
  const dim3 grid((unsigned)nb), block(NW * 64);
  if (args.dbg && !pre)
    hipLaunchKernelGGL((attn_kernel<NW, KT, true, true, false, NBUF>), grid, block, 0, s, args);
  else if (!use_tr)
    hipLaunchKernelGGL((attn_kernel<NW, KT, false, false, false, NBUF>), grid, block, 0, s, args);
  else if (pre)
    hipLaunchKernelGGL((attn_kernel<NW, KT, true, false, true, NBUF>), grid, block, 0, s, args);
  else
    hipLaunchKernelGGL((attn_kernel<NW, KT, true, false, false, NBUF>), grid, block, 0, s, args);
  return seva_check_launch("attn_kernel");
}

// Whether 32 < lq <= 64, lk <= 64 takes the two-wave one-buffer kernel when knob attn_short2 is unset (the A/B: DESIGN.md §5,
// profiles/long_window.log, tools/klong_window_time.py).
constexpr bool kAttnShort2Default = false;

}  // namespace

// attn_combine_kernel for the K/V-split fp8 P.V kernel (attention_fp8.hip: attn_write_partial16's layout, as attn16_kernel<64, true>)
int seva_attn_combine_launch(const float* part_o, const float* part_ml, int nsplit, void* out, int64_t o_sb0, int64_t o_sb1,
                             int64_t o_sl, int nb1, int heads, int lq, int64_t rows_all, hipStream_t s) {
  AttnArgs a{};
  a.out = (half_t*)out;
  a.o_sb0 = o_sb0; a.o_sb1 = o_sb1; a.o_sl = o_sl;
  a.nb1 = nb1; a.heads = heads; a.lq = lq;
  a.part_o = (float*)part_o; a.part_ml = (float*)part_ml; a.nsplit = nsplit;
  hipLaunchKernelGGL(attn_combine_kernel, dim3((unsigned)((rows_all * 8 + 255) / 256)), dim3(256), 0, s, a, rows_all);
  return seva_check_launch("attn_combine_kernel");
}

extern "C" int seva_attention_f16(const seva_attn_desc* d, seva_stream_t stream) {
  if (int rc = attn_check_desc(d, "attention", true)) return rc;
  if (int rc = attn_check_ptrs("attention", {d->q, d->k, d->v, d->out})) return rc;
  AttnArgs a{};
  attn_fill_base(a, d);
  a.v = (const half_t*)d->v;
  a.scale_log2 = d->scale * 1.44269504088896340736f;
  a.dbg = g_seva_knobs.attn_dbg > 0 ? g_seva_knobs.attn_dbg : 0;
  const int64_t batch = (int64_t)d->nb0 * d->nb1;
  const bool use_tr = g_seva_knobs.attn_no_tr != 1;  // knob attn_no_tr = 1: scalar LDS reads instead of tr_b16 (debug)
  hipStream_t s = (hipStream_t)stream;
  const double flops = 4.0 * (double)batch * d->heads * (double)d->lq * (double)d->lk * 64.0;
  const double alg_bytes = (double)batch * d->heads * 64.0 * 2.0 * (2.0 * (double)d->lq + 2.0 * (double)d->lk);  // q, out, k, v
  SevaProfScope prof(2, flops, s, alg_bytes);
  const bool pre = d->q_prescaled != 0;
  SEVA_REQUIRE(!pre || use_tr, "attention: q_prescaled is not available on the SEVA_ATTN_NO_TR debug path");
  if (d->lq <= 32) return launch<1, 32>(a, batch, s, use_tr, pre);
  // Short sequences past one wave (32 < lq <= 64, lk <= 64: the temporal regime of a 33..64-frame window): two waves, one K/V tile
  // in ONE buffer.  attn_kernel<4, 64> gives such a launch four waves of which two own no query row, and 48 KiB of LDS for a ring
  // that never turns.  Each of the two waves does what the same wave of attn_kernel<4, 64> does, on the same LDS image: equal bits
  // (tests/test_long_window_gpu.py).  Knob attn_short2: 1 = this route, 0 = attn_kernel<4, 64>; unset = kAttnShort2Default.
  if (d->lq <= 64 && d->lk <= 64 && (g_seva_knobs.attn_short2 < 0 ? kAttnShort2Default : g_seva_knobs.attn_short2 == 1))
    return launch<2, 64, 1>(a, batch, s, use_tr, pre);
  // Long sequences (lq >= SEVA_ATTN_LONG_MIN_LQ): 64 queries per wave, K / V fragments shared by all its query blocks.  Default: attn16_kernel
  // (v_mfma_f32_16x16x32; -3 ... -7 % against attn2_kernel on the long shapes of a step, same-box, profiles/r04_kattn16.log).
  // Knob attn_two: 0 forces attn_kernel, 1 / 2 select attn2_kernel (v_mfma_f32_32x32x16, bitwise equal to attn_kernel) from
  // lq >= 512, 4 selects attn16_kernel from lq >= 512.
  const int two = g_seva_knobs.attn_two;
  if (pre && use_tr && !a.dbg && ((two < 0 && d->lq >= SEVA_ATTN_LONG_MIN_LQ) || ((two == 1 || two == 2 || two == 4) && d->lq >= 512))) {
    const bool k16 = two == 4 || two < 0;
    const int qrows = 256;
    AttnArgs args = a;
    args.qblocks = (a.lq + qrows - 1) / qrows;
    const int64_t nb = batch * a.heads * args.qblocks;
    if (int rc = attn_check_grid("attention", nb)) return rc;
    // K/V split (seva_attn_desc.split_ws): two workgroups per query block for long key sequences.  The factor is a function of
    // lk alone (never of the batch); knob attn_split: 0 = never, 2..4 = that factor wherever a workspace is given.
    int nsplit = d->lk >= SEVA_ATTN_SPLIT_MIN_LK ? 2 : 1;
    if (g_seva_knobs.attn_split >= 0) nsplit = g_seva_knobs.attn_split > 4 ? 4 : g_seva_knobs.attn_split;
    const int nt_all = (d->lk + 63) / 64;
    while (nsplit >= 2 && (nt_all + nsplit - 1) / nsplit * (nsplit - 1) >= nt_all) --nsplit;  // every split gets >= 1 tile
    if (nsplit >= 2 && d->split_ws != nullptr) {
      const int64_t rows_all = batch * a.heads * (int64_t)a.lq;
      if (int rc = attn_split_setup(args, d, "attention", nsplit, rows_all, nb)) return rc;
      if (k16) hipLaunchKernelGGL((attn16_kernel<64, true>), dim3((unsigned)(nb * nsplit)), dim3(256), 0, s, args);
      else hipLaunchKernelGGL((attn2_kernel<64, true>), dim3((unsigned)(nb * nsplit)), dim3(256), 0, s, args);
      int rc = seva_check_launch("attn16_kernel / attn2_kernel <split>");
      if (rc) return rc;
      hipLaunchKernelGGL(attn_combine_kernel, dim3((unsigned)((rows_all * 8 + 255) / 256)), dim3(256), 0, s, args, rows_all);
      return seva_check_launch("attn_combine_kernel");
    }
    if (k16) hipLaunchKernelGGL((attn16_kernel<64>), dim3((unsigned)nb), dim3(256), 0, s, args);
    else hipLaunchKernelGGL((attn2_kernel<64>), dim3((unsigned)nb), dim3(256), 0, s, args);
    return seva_check_launch("attn16_kernel / attn2_kernel");
  }
  return launch<4, 64>(a, batch, s, use_tr, pre);
}
