// Opt-in fp8 P.V attention of the fp8 precision mode (Seva.set_precision("fp8", attention="fp8")): the long-sequence launches that
// seva_attention_f16 sends to attn16_kernel (lq >= SEVA_ATTN_LONG_MIN_LQ), with the P.V half of the MFMA work on v_mfma_scale_f32_16x16x128_f8f6f4.
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
// Every tiling decision is a function of lk and per-sample sizes only (K/V split from lk >= SEVA_ATTN_SPLIT_MIN_LK, as seva_attention_f16).
#include "attn_common.h"
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

struct Pv8Args : AttnBase {
  const uint8_t* v8;
  const uint8_t* v8s;
  int32_t nsteps;
};

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
  typedef AttnRing<KT, NW, BUF_BYTES, nullptr> KRing;  // the K rows; this kernel copies its own V image and scales
  constexpr int IPV = V_BYTES / 1024 / NW;    // 1 KB V instructions per wave per tile
  constexpr int G = KRing::G + IPV + 1;       // LDS-DMA instructions per wave per tile (+ the scale dwords)
  constexpr float RESCALE_THR = 8.0f;         // P <= 2^8 < 448
  // scores are computed, tested and packed in NPART parts of the tile (the registers of all 128 scores of four query blocks do not fit)
  constexpr int NPART = 4, KBP = KT / 16 / NPART;
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
  const int64_t step0 = ((int64_t)w.batch * p.heads + w.head) * p.nsteps + w.key0 / KT;
  const uint8_t* vp = p.v8 + step0 * V_BYTES + (wave * IPV) * 1024 + lane * 16;
  const uint8_t* sp8 = p.v8s + step0 * PV8_SCALE_BYTES + lane * 4;
  half_t* const obase = attn_o_base(p, w);

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
  KRing kring(kbase, nullptr, p.k_sl, lk, smem, lane, wave);
  auto issue_tile = [&](int kt, int buf) {  // tiles are issued strictly in order 0, 1, 2, ...
    kring(kt, buf);  // (rows past lk read the last key: their scores are masked; their V positions are zero in the image)
    const unsigned base = kring.smem_base + buf * BUF_BYTES;
#pragma unroll
    for (int i = 0; i < IPV; ++i) glds16_raw(vp + i * 1024, base + K_BYTES + (kring.wave_u * IPV + i) * 1024);
    glds4(sp8, base + K_BYTES + V_BYTES + kring.wave_u * PV8_SCALE_BYTES);
    vp += V_BYTES;
    sp8 += PV8_SCALE_BYTES;
  };
  const v8i_t ones = {0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838};  // e4m3 1.0

  auto tile = [&](int buf, auto masked_c, int kt) {
    constexpr bool MASKED = decltype(masked_c)::value;
    const char* const lds_k = smem + buf * BUF_BYTES;
    const char* const lds_v = lds_k + K_BYTES;
    const bool more2 = attn_ring_prefetch(kt, nt, buf, true, issue_tile);

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
            const half8_t kf = *(const half8_t*)(lds_k + krow * 128 + (k_chunk_swz(krow, 4 * ks + g) << 4));
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
    attn_ring_arrive<G>(more2);
  };
  // (attn_ring_start written out: through the function hipcc allocates this kernel three SGPRs fewer, and its registers are to stay)
  issue_tile(0, 0);
  if (nt > 1) {
    issue_tile(1, 1);
    wait_vm<G>();
  } else {
    wait_vm<0>();
  }
  attn_retire_loads(qf);
  __syncthreads();
  const int nfull = lk / KT;
  int buf = 0;
  for (int kt = 0; kt < nfull; ++kt) {
    tile(buf, std::false_type{}, kt);
    buf = buf == 2 ? 0 : buf + 1;
  }
  if (nfull < nt) tile(buf, std::true_type{}, nfull);

  // the ones-MFMA leaves the full row sum of query i16 in every register of every lane of it
  float l_tot[NQ];
#pragma unroll
  for (int c = 0; c < NQ; ++c) l_tot[c] = acc_l[c][0];
  if constexpr (SPLIT) {
    attn_write_partial16(p, w, wq0, acc_o, m_run, l_tot, i16, g);
    return;
  }
  attn_store_o16(smem, obase, p.o_sl, wq0, p.lq, acc_o, l_tot, lane, wave, i16, g);
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
  if (int rc = attn_check_desc(d, "attn_quant_v_fp8", false)) return rc;
  if (int rc = attn_check_ptrs("attn_quant_v_fp8", {d->v, v8, v8_scale})) return rc;
  const int64_t batch = (int64_t)d->nb0 * d->nb1, nsteps = pv8_steps(d->lk);
  const int64_t nb = batch * d->heads * nsteps;
  if (int rc = attn_check_grid("attn_quant_v_fp8", nb)) return rc;
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
  if (int rc = attn_check_desc(d, "attention_pv8", true)) return rc;
  if (int rc = attn_check_ptrs("attention_pv8", {d->q, d->k, v8, v8_scale, d->out})) return rc;
  SEVA_REQUIRE(d->q_prescaled != 0, "attention_pv8: q must be pre-scaled by scale * log2(e) (q_prescaled)");
  const int64_t batch = (int64_t)d->nb0 * d->nb1;
  Pv8Args a{};
  attn_fill_base(a, d);
  a.v8 = (const uint8_t*)v8; a.v8s = v8_scale;
  a.qblocks = (d->lq + 255) / 256;
  a.nsteps = pv8_steps(d->lk);
  const int64_t nb = batch * d->heads * a.qblocks;
  if (int rc = attn_check_grid("attention_pv8", nb)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const double flops = 4.0 * (double)batch * d->heads * (double)d->lq * (double)d->lk * 64.0;
  const double alg_bytes = (double)batch * d->heads * 64.0 * (2.0 * 2.0 * (double)d->lq + 3.0 * (double)d->lk);  // q, out f16; k f16, v e4m3
  SevaProfScope prof(2, flops, s, alg_bytes);
  // K/V split as seva_attention_f16 (split_ws; a function of lk alone), counted in 128-key tiles
  int nsplit = d->lk >= SEVA_ATTN_SPLIT_MIN_LK ? 2 : 1;
  const int nt_all = pv8_steps(d->lk);
  while (nsplit >= 2 && (nt_all + nsplit - 1) / nsplit * (nsplit - 1) >= nt_all) --nsplit;  // every split gets >= 1 tile
  if (nsplit >= 2 && d->split_ws != nullptr) {
    const int64_t rows_all = batch * d->heads * (int64_t)d->lq;
    if (int rc = attn_split_setup(a, d, "attention_pv8", nsplit, rows_all, nb)) return rc;
    hipLaunchKernelGGL((pv8_kernel<true>), dim3((unsigned)(nb * nsplit)), dim3(256), 0, s, a);
    if (int rc = seva_check_launch("pv8_kernel <split>")) return rc;
    return seva_attn_combine_launch(a.part_o, a.part_ml, nsplit, d->out, d->o_sb0, d->o_sb1, d->o_sl, d->nb1, d->heads, d->lq,
                                    rows_all, s);
  }
  hipLaunchKernelGGL((pv8_kernel<false>), dim3((unsigned)nb), dim3(256), 0, s, a);
  return seva_check_launch("pv8_kernel");
}
