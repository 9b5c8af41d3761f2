// Opt-in fp8 P.V attention of the fp8 precision mode (Seva.set_precision("fp8", attention="fp8")): the long-sequence launches that
// seva_attention_f16 sends to attn16_kernel (lq >= 2048), with the P.V half of the MFMA work on v_mfma_scale_f32_16x16x128_f8f6f4.
//
//   quant_v_fp8_kernel  V (f16, the attention descriptor's strides) -> e4m3 V^T in the kernel's key order + E8M0 scale per 32 keys and
//                       channel (layout: attn_pv8.h)
//   pv8_kernel          attn16_kernel's scheme (4 waves x 64 queries as four 16-row blocks, K / V^T fragments shared by the four blocks,
//                       3-deep LDS-DMA ring, q pre-scaled by scale * log2(e)) with 128-key tiles:
//                         S^T = K Q^T on v_mfma_f32_16x16x32_f16 exactly as there, in four 32-key parts
//                         P = exp2(S - m_run) packed to e4m3 in registers as it sits = the B operand of the scaled MFMA (unit scale)
//                         O^T += V^T P^T, A operand = the quantised V^T tile with its E8M0 scales (one MFMA per 128 keys, 16 dims, 16 queries)
//                         l   += 1^T P^T, the same MFMA with an all-ones A operand: the row sum is taken from the QUANTISED P, so numerator
//                               and normaliser see identical probabilities (as the f16 kernels sum their rounded f16 P)
// The overflow trap: attn16 lets a probability grow to 2^14 before it rescales; e4m3 ends at 448.  Here the rescale test is the score
// itself (attn_kernel's rule with RESCALE_THR = 8): whenever a score of a 32-key part exceeds m_run + 8 the reference moves to
// ceil(running maximum) - 8, so P <= 2^8 = 256 and the row's largest P sits in the top binades of e4m3 (the small probabilities keep
// 8 binades more of normal range than with P <= 1).  The reference is INTEGER: alpha = 2^-delta is exact, and it is always exactly
// ceil(running maximum) - 8, so the e4m3 rounding of P is a function of the scores alone (e4m3(x 2^k) = e4m3(x) 2^k for integer k in
// the normal range; tests/test_attention_fp8_cpu.py: pv8_reference).  A rescale in a later part of a tile first accumulates the
// earlier parts' packed P (a second, rare, set of MFMAs) -- they were packed against the old reference.
// Every tiling decision is a function of lk and per-sample sizes only (K/V split from lk >= 6144, as seva_attention_f16).
#include <type_traits>

#include "attn_pv8.h"

namespace {

typedef int v8i_t __attribute__((ext_vector_type(8)));
typedef int v4i_t __attribute__((ext_vector_type(4)));

struct QuantArgs {
  const half_t* v;
  uint8_t* v8;
  uint8_t* v8s;
  int64_t sb0, sb1, sl;
  int32_t nb1, heads, lk, nsteps;
};

// one workgroup per (batch, head, step); thread (channel d = tid & 63, scale group b = tid >> 6) owns positions 32 g + 16 (b >> 1) .. +15 of
// the two lane groups g = 2 (b & 1), 2 (b & 1) + 1 (attn_pv8.h)
__global__ __launch_bounds__(256) void quant_v_fp8_kernel(QuantArgs p) {
  const int64_t id = blockIdx.x;  // ((batch * heads) + head) * nsteps + step
  const int step = (int)(id % p.nsteps);
  const int64_t bh = id / p.nsteps;
  const int head = (int)(bh % p.heads);
  const int64_t batch = bh / p.heads;
  const int64_t b0 = batch / p.nb1, b1 = batch - b0 * p.nb1;
  const half_t* const vb = p.v + b0 * p.sb0 + b1 * p.sb1 + head * 64;
  const int d = threadIdx.x & 63, b = threadIdx.x >> 6;
  float x[32];
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int key = step * PV8_STEP + pv8_key_of(pv8_group_pos(b, j));  // a wave reads one 128-byte key row per j
    x[j] = key < p.lk ? (float)vb[(int64_t)key * p.sl + d] : 0.f;
    amax = fmaxf(amax, fabsf(x[j]));
  }
  // smallest e with amax * 2^-e <= 448 = 0.875 * 2^9: amax = m 2^E, m in [0.5, 1)
  int E;
  const float m = frexpf(fmaxf(amax, 1e-30f), &E);
  int e = m <= 0.875f ? E - 9 : E - 8;
  e = e < -126 ? -126 : (e > 127 ? 127 : e);
  int w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
    w[i] = pack_fp8x4(ldexpf(x[4 * i], -e), ldexpf(x[4 * i + 1], -e), ldexpf(x[4 * i + 2], -e), ldexpf(x[4 * i + 3], -e));
  uint8_t* const row = p.v8 + id * PV8_VALUE_BYTES + d * 128;
  *(v4i_t*)(row + (pv8_chunk_swz(d, pv8_group_pos(b, 0) >> 4) << 4)) = v4i_t{w[0], w[1], w[2], w[3]};
  *(v4i_t*)(row + (pv8_chunk_swz(d, pv8_group_pos(b, 16) >> 4) << 4)) = v4i_t{w[4], w[5], w[6], w[7]};
  p.v8s[id * PV8_SCALE_BYTES + pv8_scale_index(d, b)] = (uint8_t)(127 + e);
}

struct Pv8Args {
  const half_t* q;
  const half_t* k;
  const uint8_t* v8;
  const uint8_t* v8s;
  half_t* out;
  int64_t q_sb0, q_sb1, q_sl;
  int64_t k_sb0, k_sb1, k_sl;
  int64_t o_sb0, o_sb1, o_sl;
  int32_t nb1, heads, lq, lk, qblocks, nsteps;
  float* part_o;   // K/V split: [nsplit][batch * heads * lq][64]   (attn16_kernel's layout, read by attn_combine_kernel)
  float* part_ml;  //            [nsplit][batch * heads * lq][2]
  int32_t nsplit;
};

// LDS-DMA from inline asm, ordered only by the counted waits and barriers (as attention.hip)
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_wave_base) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_wave_base)
               : "memory");
}
__device__ __forceinline__ void glds4(const void* gsrc, unsigned lds_wave_base) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_wave_base)
               : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ int k_swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }  // attn16_kernel's K tile swizzle

// O^T block (16 dims x 16 queries) += V^T (16 dims x 128 keys, e4m3, E8M0 byte SEL of vscale) * P^T (128 keys x 16 queries, e4m3, unit scale)
template <int SEL>
__device__ __forceinline__ f32x4 mfma_pv(v8i_t v, v8i_t pf, f32x4 c, int vscale) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(v, pf, c, 0 /*e4m3*/, 0 /*e4m3*/, SEL, vscale, 0, 0x7F7F7F7F);
}

template <bool SPLIT>
__global__ __launch_bounds__(256, 2) void pv8_kernel(Pv8Args p) {
  constexpr int KT = PV8_STEP, NW = 4, NQ = 4;
  constexpr int K_BYTES = KT * 128, V_BYTES = PV8_VALUE_BYTES, S_BYTES = NW * PV8_SCALE_BYTES;  // every wave stages its own scale copy
  constexpr int BUF_BYTES = K_BYTES + V_BYTES + S_BYTES;
  __shared__ __attribute__((aligned(16))) char smem[3 * BUF_BYTES];
  constexpr int IPK = KT / 8 / NW;            // 8-row K instructions per wave per tile
  constexpr int IPV = V_BYTES / 1024 / NW;    // 1 KB V instructions per wave per tile
  constexpr int G = IPK + IPV + 1;            // LDS-DMA instructions per wave per tile (+ the scale dwords)
  constexpr float RESCALE_THR = 8.0f;         // P <= 2^8 < 448
  // scores are computed, tested and packed in NPART parts of the tile (the registers of all 128 scores of four query blocks do not fit)
  constexpr int NPART = 4, KBP = KT / 16 / NPART;
  static_assert(3 * BUF_BYTES >= NW * 64 * 128, "the output staging re-uses the ring");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;

  int bid;
  {
    const int nb = gridDim.x, q = nb >> 3, r = nb & 7, x = blockIdx.x & 7;
    bid = ((x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (blockIdx.x >> 3);
  }
  const int qb = bid % p.qblocks;
  bid /= p.qblocks;
  int ksp = 0;
  if (SPLIT) {
    ksp = bid % p.nsplit;
    bid /= p.nsplit;
  }
  const int head = bid % p.heads;
  const int batch = bid / p.heads;
  const int b0 = batch / p.nb1, b1 = batch - b0 * p.nb1;
  int key0 = 0, lk = p.lk;
  if (SPLIT) {
    const int nt_all = (p.lk + KT - 1) / KT, tps = (nt_all + p.nsplit - 1) / p.nsplit;
    key0 = ksp * tps * KT;
    const int key1 = (ksp + 1) * tps * KT < p.lk ? (ksp + 1) * tps * KT : p.lk;
    lk = key1 - key0;  // > 0: the host only splits when every split gets at least one tile
  }

  const half_t* const qbase = p.q + b0 * p.q_sb0 + b1 * p.q_sb1 + head * 64;
  const half_t* const kbase = p.k + b0 * p.k_sb0 + b1 * p.k_sb1 + head * 64 + (int64_t)key0 * p.k_sl;
  const int64_t step0 = ((int64_t)batch * p.heads + head) * p.nsteps + key0 / KT;
  const uint8_t* vp = p.v8 + step0 * V_BYTES + (wave * IPV) * 1024 + lane * 16;
  const uint8_t* sp8 = p.v8s + step0 * PV8_SCALE_BYTES + lane * 4;
  half_t* const obase = p.out + b0 * p.o_sb0 + b1 * p.o_sb1 + head * 64;

  const int wq0 = qb * (64 * NW) + wave * 64;
  half8_t qf[NQ][2];
#pragma unroll
  for (int c = 0; c < NQ; ++c) {
    const int qrow = wq0 + 16 * c + i16;
    const int qrow_c = qrow < p.lq ? qrow : p.lq - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[c][ks] = *(const half8_t*)(qbase + (int64_t)qrow_c * p.q_sl + 32 * ks + 8 * g);
  }
  const bool active = __builtin_amdgcn_readfirstlane(wq0) < p.lq;
  f32x4 acc_o[NQ][4], acc_l[NQ];
  float m_run[NQ];
  f32x4 neg_m[NQ];
#pragma unroll
  for (int c = 0; c < NQ; ++c) {
    m_run[c] = 0.f;
    neg_m[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc_l[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < 4; ++d) acc_o[c][d] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int nt = (lk + KT - 1) / KT;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const unsigned smem_base =
      __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem);
  const int sr = lane >> 3, sc8 = lane & 7;
  const half_t* kp[IPK];
#pragma unroll
  for (int i = 0; i < IPK; ++i) {
    const int row = 8 * (wave_u * IPK + i) + sr;
    const int key = row < lk ? row : lk - 1;
    kp[i] = kbase + (int64_t)key * p.k_sl + k_swz(row, sc8) * 8;
  }
  const int64_t tile_stride = (int64_t)KT * p.k_sl;
  const bool ragged = (lk % KT) != 0;
  auto issue_tile = [&](int kt, int buf) {  // tiles are issued strictly in order 0, 1, 2, ...
    const bool clamp = ragged && kt == nt - 1 && kt > 0;
    const unsigned base = smem_base + buf * BUF_BYTES;
#pragma unroll
    for (int i = 0; i < IPK; ++i) {
      const unsigned dst = base + 8 * (wave_u * IPK + i) * 128;
      if (clamp) {  // rows past lk read the last key (their scores are masked; their V positions are zero in the image)
        const int row = 8 * (wave_u * IPK + i) + sr;
        int key = kt * KT + row;
        if (key >= lk) key = lk - 1;
        glds16(kbase + (int64_t)key * p.k_sl + k_swz(row, sc8) * 8, dst);
      } else {
        glds16(kp[i], dst);
      }
      kp[i] += tile_stride;
    }
#pragma unroll
    for (int i = 0; i < IPV; ++i) glds16(vp + i * 1024, base + K_BYTES + (wave_u * IPV + i) * 1024);
    glds4(sp8, base + K_BYTES + V_BYTES + wave_u * PV8_SCALE_BYTES);
    vp += V_BYTES;
    sp8 += PV8_SCALE_BYTES;
  };
  const v8i_t ones = {0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838};  // e4m3 1.0

  auto tile = [&](int buf, auto masked_c, int kt) {
    constexpr bool MASKED = decltype(masked_c)::value;
    const char* const lds_k = smem + buf * BUF_BYTES;
    const char* const lds_v = lds_k + K_BYTES;
    const bool more2 = kt + 2 < nt;
    if (more2) issue_tile(kt + 2, buf == 0 ? 2 : buf - 1);  // (buf + 2) % 3

    if (active) {
      // this lane's V^T row 16 db + i16, positions [32 g, 32 g + 32): two b128 reads
      const auto read_v = [&](int db) {
        const int row = 16 * db + i16;
        const v4i_t lo = *(const v4i_t*)(lds_v + row * 128 + (pv8_chunk_swz(row, 2 * g) << 4));
        const v4i_t hi = *(const v4i_t*)(lds_v + row * 128 + (pv8_chunk_swz(row, 2 * g + 1) << 4));
        return v8i_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      };
      const auto pv = [&](int c, const v8i_t (&vf)[4], v8i_t pc, int vs) {
        acc_o[c][0] = mfma_pv<0>(vf[0], pc, acc_o[c][0], vs);
        acc_o[c][1] = mfma_pv<1>(vf[1], pc, acc_o[c][1], vs);
        acc_o[c][2] = mfma_pv<2>(vf[2], pc, acc_o[c][2], vs);
        acc_o[c][3] = mfma_pv<3>(vf[3], pc, acc_o[c][3], vs);
        acc_l[c] = mfma_pv<0>(ones, pc, acc_l[c], 0x7F7F7F7F);
      };
      const int vs = *(const int*)(lds_v + V_BYTES + wave * PV8_SCALE_BYTES + lane * 4);
      v8i_t pf[NQ];
#pragma unroll
      for (int h = 0; h < NPART; ++h) {
        // ---- S^T = K Q^T for the part's key blocks and the four query blocks off ONE K fragment (attn16_kernel's) ----
        __builtin_amdgcn_sched_barrier(0);  // one part's scores live at a time
        f32x4 sc[NQ][KBP];
#pragma unroll
        for (int kk = 0; kk < KBP; ++kk) {
          const int krow = 16 * (KBP * h + kk) + i16;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const half8_t kf = *(const half8_t*)(lds_k + krow * 128 + (k_swz(krow, 4 * ks + g) << 4));
#pragma unroll
            for (int c = 0; c < NQ; ++c)
              sc[c][kk] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[c][ks], ks == 0 ? neg_m[c] : sc[c][kk], 0, 0, 0);
          }
        }
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
          if (MASKED) {
#pragma unroll
            for (int kk = 0; kk < KBP; ++kk)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (kt * KT + 16 * (KBP * h + kk) + 4 * g + r >= lk) sc[c][kk][r] = -1e30f;
          }
          float mx = sc[c][0][0];
#pragma unroll
          for (int kk = 0; kk < KBP; ++kk)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sc[c][kk][r]);
          const bool first = kt == 0 && h == 0;
          if (__builtin_expect(first || __any(!(mx <= RESCALE_THR)), 0)) {  // wave-uniform, rare (NaN lands here too)
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));  // the four lanes of a query
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            if (h > 0) {  // the earlier parts are packed against the old reference: accumulate them now, alone (one V^T block at a time)
              v8i_t p0;
#pragma unroll
              for (int j = 0; j < 8; ++j) p0[j] = j < KBP * h ? pf[c][j] : 0;
              acc_o[c][0] = mfma_pv<0>(read_v(0), p0, acc_o[c][0], vs);
              acc_o[c][1] = mfma_pv<1>(read_v(1), p0, acc_o[c][1], vs);
              acc_o[c][2] = mfma_pv<2>(read_v(2), p0, acc_o[c][2], vs);
              acc_o[c][3] = mfma_pv<3>(read_v(3), p0, acc_o[c][3], vs);
              acc_l[c] = mfma_pv<0>(ones, p0, acc_l[c], 0x7F7F7F7F);
#pragma unroll
              for (int j = 0; j < KBP * h; ++j) pf[c][j] = 0;
            }
            // the reference becomes ceil(running maximum) - 8: P <= 2^8 stays in e4m3's range, the largest P of the row in [2^7, 2^8]
            const float delta = first ? ceilf(mx) - RESCALE_THR : fmaxf(ceilf(mx) - RESCALE_THR, 0.f);  // integer
            const float alpha = first ? 1.0f : __builtin_amdgcn_exp2f(-delta);                        // exact power of two
            m_run[c] += delta;
#pragma unroll
            for (int r = 0; r < 4; ++r) neg_m[c][r] = -m_run[c];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc_l[c][r] *= alpha;
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
              for (int r = 0; r < 4; ++r) acc_o[c][d][r] *= alpha;
#pragma unroll
            for (int kk = 0; kk < KBP; ++kk)
#pragma unroll
              for (int r = 0; r < 4; ++r) sc[c][kk][r] -= delta;
          }
          // P in [0, 256]: e4m3 without saturation; byte r of dword kb = key 16 kb + 4 g + r (attn_pv8.h)
#pragma unroll
          for (int kk = 0; kk < KBP; ++kk) {
            int w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_exp2f(sc[c][kk][0]), __builtin_amdgcn_exp2f(sc[c][kk][1]), 0, false);
            pf[c][KBP * h + kk] =
                __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_exp2f(sc[c][kk][2]), __builtin_amdgcn_exp2f(sc[c][kk][3]), w, true);
          }
        }
      }
      // ---- O^T += V^T P^T and l += 1^T P^T for the four query blocks off ONE V^T fragment set ----
      const v8i_t vf[4] = {read_v(0), read_v(1), read_v(2), read_v(3)};
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < NQ; ++c) pv(c, vf, pf[c], vs);
    }  // active
    if (more2) wait_vm<G>();
    else wait_vm<0>();
    __syncthreads();
  };

  issue_tile(0, 0);
  if (nt > 1) {
    issue_tile(1, 1);
    wait_vm<G>();
  } else {
    wait_vm<0>();
  }
#pragma unroll
  for (int c = 0; c < NQ; ++c)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) asm volatile("" : "+v"(qf[c][ks]));  // retire the Q loads (see attention.hip)
  __syncthreads();
  const int nfull = lk / KT;
  int buf = 0;
  for (int kt = 0; kt < nfull; ++kt) {
    tile(buf, std::false_type{}, kt);
    buf = buf == 2 ? 0 : buf + 1;
  }
  if (nfull < nt) tile(buf, std::true_type{}, nfull);

  // the ones-MFMA leaves the full row sum of query i16 in every register of every lane of it
  if constexpr (SPLIT) {
    const int64_t rows_all = (int64_t)gridDim.x / (p.qblocks * p.nsplit) * p.lq;  // batch * heads * lq
    const int64_t row_bh = ((int64_t)batch * p.heads + head) * p.lq;
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
      const int qrow = wq0 + 16 * c + i16;
      if (qrow < p.lq) {
        float* const po = p.part_o + ((int64_t)ksp * rows_all + row_bh + qrow) * 64;
#pragma unroll
        for (int db = 0; db < 4; ++db) *(f32x4*)(po + 16 * db + 4 * g) = acc_o[c][db];
        if (g == 0) {
          float* const pm = p.part_ml + ((int64_t)ksp * rows_all + row_bh + qrow) * 2;
          pm[0] = m_run[c];
          pm[1] = acc_l[c][0];
        }
      }
    }
    return;
  }
  __syncthreads();  // every wave is done reading K/V tiles
  char* const ow = smem + wave * (64 * 128);
#pragma unroll
  for (int c = 0; c < NQ; ++c) {
    const float inv = 1.0f / acc_l[c][0];
    const int row = 16 * c + i16;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      half4_t hv;
#pragma unroll
      for (int r = 0; r < 4; ++r) hv[r] = (half_t)(acc_o[c][db][r] * inv);
      const int d0 = 16 * db + 4 * g;
      const int chunk = d0 >> 3, piece = (d0 >> 2) & 1;
      *(half4_t*)(ow + row * 128 + ((chunk ^ (row & 7)) << 4) + (piece << 3)) = hv;
    }
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): same wave reads back its own image
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = 8 * i + (lane >> 3), pchunk = lane & 7;
    const uint4 v = *(const uint4*)(ow + row * 128 + (pchunk << 4));
    const int lchunk = pchunk ^ (row & 7);
    if (wq0 + row < p.lq) *(uint4*)(obase + (int64_t)(wq0 + row) * p.o_sl + lchunk * 8) = v;
  }
}

int check_desc(const seva_attn_desc* d, const char* what) {
  SEVA_REQUIRE(d != nullptr, "%s: null desc", what);
  SEVA_REQUIRE(d->lq > 0 && d->lk > 0 && d->heads > 0 && d->nb0 > 0 && d->nb1 > 0,
               "%s: empty problem lq=%d lk=%d heads=%d nb=%dx%d", what, d->lq, d->lk, d->heads, d->nb0, d->nb1);
  SEVA_REQUIRE((d->k_sb0 | d->k_sb1 | d->k_sl) % 8 == 0, "%s: strides must be multiples of 8 elements", what);
  return SEVA_OK;
}

}  // namespace

extern "C" int seva_attn_v_fp8_size(int32_t batch, int32_t heads, int32_t lk, int64_t* v8_bytes, int64_t* scale_bytes) {
  SEVA_REQUIRE(batch > 0 && heads > 0 && lk > 0 && v8_bytes && scale_bytes, "attn_v_fp8_size: bad arguments batch=%d heads=%d lk=%d",
               batch, heads, lk);
  const int64_t steps = (int64_t)batch * heads * pv8_steps(lk);
  *v8_bytes = steps * PV8_VALUE_BYTES;
  *scale_bytes = steps * PV8_SCALE_BYTES;
  return SEVA_OK;
}

extern "C" int seva_attn_quant_v_fp8(const seva_attn_desc* d, void* v8, uint8_t* v8_scale, seva_stream_t stream) {
  if (int rc = check_desc(d, "attn_quant_v_fp8")) return rc;
  SEVA_REQUIRE(d->v && v8 && v8_scale, "attn_quant_v_fp8: null pointer");
  SEVA_REQUIRE(((uintptr_t)d->v | (uintptr_t)v8 | (uintptr_t)v8_scale) % 16 == 0, "attn_quant_v_fp8: pointers must be 16-byte aligned");
  const int64_t batch = (int64_t)d->nb0 * d->nb1, nsteps = pv8_steps(d->lk);
  const int64_t nb = batch * d->heads * nsteps;
  SEVA_REQUIRE(nb <= 0x7fffffff, "attn_quant_v_fp8: bad grid %lld", (long long)nb);
  QuantArgs a{};
  a.v = (const half_t*)d->v;
  a.v8 = (uint8_t*)v8;
  a.v8s = v8_scale;
  a.sb0 = d->k_sb0; a.sb1 = d->k_sb1; a.sl = d->k_sl;
  a.nb1 = d->nb1; a.heads = d->heads; a.lk = d->lk; a.nsteps = (int32_t)nsteps;
  hipStream_t s = (hipStream_t)stream;
  SevaProfScope prof(2, 0.0, s, (double)batch * d->heads * d->lk * 64.0 * 3.0);
  hipLaunchKernelGGL(quant_v_fp8_kernel, dim3((unsigned)nb), dim3(256), 0, s, a);
  return seva_check_launch("quant_v_fp8_kernel");
}

extern "C" int seva_attention_pv8(const seva_attn_desc* d, const void* v8, const uint8_t* v8_scale, seva_stream_t stream) {
  if (int rc = check_desc(d, "attention_pv8")) return rc;
  SEVA_REQUIRE(d->q && d->k && v8 && v8_scale && d->out, "attention_pv8: null pointer");
  SEVA_REQUIRE(((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)v8 | (uintptr_t)v8_scale | (uintptr_t)d->out) % 16 == 0,
               "attention_pv8: pointers must be 16-byte aligned");
  SEVA_REQUIRE((d->q_sb0 | d->q_sb1 | d->q_sl | d->o_sb0 | d->o_sb1 | d->o_sl) % 8 == 0,
               "attention_pv8: strides must be multiples of 8 elements");
  SEVA_REQUIRE(d->q_prescaled != 0, "attention_pv8: q must be pre-scaled by scale * log2(e) (q_prescaled)");
  const int64_t batch = (int64_t)d->nb0 * d->nb1;
  Pv8Args a{};
  a.q = (const half_t*)d->q; a.k = (const half_t*)d->k;
  a.v8 = (const uint8_t*)v8; a.v8s = v8_scale;
  a.out = (half_t*)d->out;
  a.q_sb0 = d->q_sb0; a.q_sb1 = d->q_sb1; a.q_sl = d->q_sl;
  a.k_sb0 = d->k_sb0; a.k_sb1 = d->k_sb1; a.k_sl = d->k_sl;
  a.o_sb0 = d->o_sb0; a.o_sb1 = d->o_sb1; a.o_sl = d->o_sl;
  a.nb1 = d->nb1; a.heads = d->heads; a.lq = d->lq; a.lk = d->lk;
  a.qblocks = (d->lq + 255) / 256;
  a.nsteps = pv8_steps(d->lk);
  const int64_t nb = batch * d->heads * a.qblocks;
  SEVA_REQUIRE(nb > 0 && nb <= 0x7fffffff, "attention_pv8: bad grid %lld", (long long)nb);
  hipStream_t s = (hipStream_t)stream;
  const double flops = 4.0 * (double)batch * d->heads * (double)d->lq * (double)d->lk * 64.0;
  const double alg_bytes = (double)batch * d->heads * 64.0 * (2.0 * 2.0 * (double)d->lq + 3.0 * (double)d->lk);  // q, out f16; k f16, v e4m3
  SevaProfScope prof(2, flops, s, alg_bytes);
  // K/V split as seva_attention_f16 (split_ws; a function of lk alone), counted in 128-key tiles
  int nsplit = d->lk >= 6144 ? 2 : 1;
  const int nt_all = pv8_steps(d->lk);
  while (nsplit >= 2 && (nt_all + nsplit - 1) / nsplit * (nsplit - 1) >= nt_all) --nsplit;  // every split gets >= 1 tile
  if (nsplit >= 2 && d->split_ws != nullptr) {
    const int64_t rows_all = batch * d->heads * (int64_t)d->lq;
    SEVA_REQUIRE(d->split_ws_bytes >= nsplit * rows_all * 66 * 4 && (uintptr_t)d->split_ws % 16 == 0,
                 "attention_pv8: split_ws too small (%lld bytes, need %lld) or misaligned", (long long)d->split_ws_bytes,
                 (long long)(nsplit * rows_all * 66 * 4));
    SEVA_REQUIRE(nb * nsplit <= 0x7fffffff && rows_all * 8 / 256 + 1 <= 0x7fffffff, "attention_pv8: split grid too large");
    a.nsplit = nsplit;
    a.part_o = d->split_ws;
    a.part_ml = d->split_ws + (int64_t)nsplit * rows_all * 64;
    hipLaunchKernelGGL((pv8_kernel<true>), dim3((unsigned)(nb * nsplit)), dim3(256), 0, s, a);
    if (int rc = seva_check_launch("pv8_kernel <split>")) return rc;
    return seva_attn_combine_launch(a.part_o, a.part_ml, nsplit, d->out, d->o_sb0, d->o_sb1, d->o_sl, d->nb1, d->heads, d->lq,
                                    rows_all, s);
  }
  hipLaunchKernelGGL((pv8_kernel<false>), dim3((unsigned)nb), dim3(256), 0, s, a);
  return seva_check_launch("pv8_kernel");
}
