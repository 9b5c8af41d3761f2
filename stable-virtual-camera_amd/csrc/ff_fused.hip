// Fused GEGLU feed-forward for the narrow (C <= 320) transformer level of the UNet:
//
//   out[m][:] = W2 . ( v * gelu_erf(g) ) + b2 (+ residual[m][:]),   [v ; g] = W1 . a[m][:] + b1
//
// i.e. FeedForward of reference seva/modules/transformer.py:18-34 (GEGLU 8-15, Linear 4C -> C) in ONE kernel.  At the
// ds1 level (C = 320, M = 217,728 token rows) the two-kernel form writes the 4C-wide hidden tensor (557 MB f16) and reads it
// back 15 times per denoising step, and both kernels re-stream their weights from L2 per 128-row tile at the L2->LDS
// rate limit; here the hidden activations never leave the registers:
//
//   * 4 waves x 32 token rows (128-row workgroup tile), ONE workgroup per CU, up to 512 registers per wave:
//       A fragments of the wave's 32 rows        (C/32 x 2 x 4 = 80 VGPRs at C = 320; loaded once),
//       stage-1 accumulators of a 64-feature hidden chunk (value + gate: 2 x 8 x 4 = 64),
//       stage-2 accumulators of the whole output row block (2 x C/16 x 4 = 160; start from the residual tile).
//   * per hidden chunk (64 features = 128 interleaved W1 rows): stage 1 = C/64 K-tiles of W1 through a 2-deep LDS ring
//     (LDS-DMA, one barrier per K-tile); GEGLU in registers; with the paired row assignment of gemm.hip a lane then
//     owns 8 consecutive hidden features of its token, which is exactly the B-operand fragment of v_mfma_f32_16x16x32_f16
//     (k = 8*(lane>>4) + j): stage 2 multiplies by the chunk's W2 slice [C rows][64 cols] (second LDS ring, staged one
//     chunk ahead, spread over the chunk's K-tiles) with no shuffle and no LDS round trip of the activations.
//   * the hidden value is rounded to f16 once (as the stored tensor was), accumulation is fp32 throughout.
//
// Weight layouts are those of seva_gemm_f16: W1 [8C][C] rows interleaved in groups of 64 = [32 value | 32 gate]
// (b1 likewise), W2 [C][4C].
#include "gemm_common.h"
#include "ff_fp8.h"

#include <atomic>

namespace {

struct FfArgs {
  const half_t* a;
  const half_t* w1;
  const float* b1;
  const half_t* w2;
  const float* b2;
  const float* residual;
  float* out_f32;
  half_t* out_f16;
  int64_t M, lda, ldr, ldo32, ldo16;
  int32_t tiles_m;
  // optional LayerNorm prologue: a = LayerNorm(ln_x) computed in registers, `a` unused
  const float* ln_x;
  const float* ln_gamma;
  const float* ln_beta;
  int64_t ldx;
  float ln_eps;
};

// e4m3 kernel (seva_ff_fused_fp8): the same arguments, `a` / w1 / w2 as e4m3 bytes (lda counts bytes), plus the weights'
// per-row E8M0 scale bytes
struct Ff8Args {
  FfArgs f;
  const uint8_t* w1_exp;
  const uint8_t* w2_exp;
};

// glds16_raw with a wave-uniform 64-bit base in SGPRs and a 32-bit per-lane byte offset (saddr form): one VGPR per staging pass
// instead of a 64-bit address pair (the e4m3 kernel runs at the register limit)
static __device__ __forceinline__ void glds16_sv(const void* sbase, unsigned voff, unsigned lds_wave_base) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_wave_base)
      : "memory");
}


// ---------------------------------------------------------------------------------------------------------------
// 8 waves on the 128-row tile, TWO waves per 32-row group (2 waves per SIMD -> one wave's LDS / barrier waits and GEGLU VALU run
// under the other's MFMAs).  Wave (mr, h): rows 32*mr .. +31; in stage 1 it takes the
// chunk's GEGLU group q = h (64 of the 128 interleaved W1 rows -> 32 hidden features), the partner's 32 features arrive
// through a 1 KiB-per-fragment LDS exchange; in stage 2 it owns output blocks h*NJ2/2 .. (half of the output row).
// Registers per wave: A 80 + stage-2 accumulators 80 + stage-1 accumulators 32 + fragments: <= 256.
// LDS rows, chunk swizzle (W1: the paired key, W2: the natural one) and the W1 row assignment are the shared tile core: gemm_tile.h.
template <int C>
__global__ __launch_bounds__(512, 2) void ff_fused8_kernel(FfArgs p) {
  constexpr int KS = C / 32, NK1 = C / 64, NJ2 = C / 16, NJH = NJ2 / 2, NCH = C / 16;
  constexpr int W1_BYTES = 128 * 128, W2_BYTES = C * 128;
  constexpr int W2_PASSES = C / 64;  // 8-row passes per wave and slice (C/8 rows per wave)
  constexpr int W2_PER_KT = (W2_PASSES + NK1 - 1) / NK1;
  static_assert(NJ2 % 2 == 0, "output blocks split over the two waves of a row group");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // [W1 ring: 3 tiles][W2 buf0][W2 buf1][b1: 8C floats][exchange: 4 row groups x 2 halves x 2 token blocks x 1 KiB]
  // W1 K-tiles form ONE sequence over all chunks (tile g = hc * NK1 + kt, buffer g % 3) staged TWO tiles ahead: the L2 ->
  // LDS latency of a tile gets two K-tiles of MFMA time, and the wait at the end of tile g is a counted vmcnt that leaves
  // the loads issued during tile g in flight (with a 2-deep ring and vmcnt(0) every K-tile paid that latency in full:
  // 12.2k cycles per chunk for 3.8k cycles of MFMA).
  constexpr int W1_RING = 3;
  char* const lds_w1 = smem;
  char* const lds_w2 = smem + W1_RING * W1_BYTES;
  float* const lds_b1 = (float*)(smem + W1_RING * W1_BYTES + 2 * W2_BYTES);
  char* const lds_x = smem + W1_RING * W1_BYTES + 2 * W2_BYTES + 8 * C * 4;
  const unsigned lds_base_u32 = __builtin_amdgcn_readfirstlane(lds_addr_u32(smem));

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int mr = wave & 3, h = wave >> 2;
  const int fr = lane & 15, fg = lane >> 4;
  const int sr = lane >> 3, sp = lane & 7;

  const int tm = xcd_remap(blockIdx.x, p.tiles_m);
  const int64_t m0 = (int64_t)tm * 128 + mr * 32;

  half8_t areg[2][KS];
  if (p.ln_x) {
    // LayerNorm prologue (reference transformer.py:102-104: x = ff(norm3(x)) + x): the wave's 32 rows are read as fp32, a
    // row lives in the 4 lanes (fr, fg = 0..3) that hold its k = 32ks + 8fg + j; exact two-pass statistics with two
    // xor-shuffles; the normalised row goes straight into the A fragments (one f16 rounding, as the LayerNorm kernel's
    // output had).  Replaces a 95 us read-4B/write-2B pass + its re-read per feed-forward at the ds1 level.
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int64_t m = m0 + 16 * i + fr;
      if (m >= p.M) m = p.M - 1;
      const float* xr = p.ln_x + m * p.ldx + 8 * fg;
      f32x4 v[KS][2];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        v[ks][0] = first_read(*(const f32x4*)(xr + 32 * ks));
        v[ks][1] = first_read(*(const f32x4*)(xr + 32 * ks + 4));
      }
      float sum = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int e = 0; e < 2; ++e) sum += v[ks][e][0] + v[ks][e][1] + v[ks][e][2] + v[ks][e][3];
      // (each cross-lane result is first read by a plain 32-bit op: see the note at the GroupNorm modulation, norm.hip)
      sum += __shfl_xor(sum, 16, 64);
      asm volatile("" : "+v"(sum));
      sum += __shfl_xor(sum, 32, 64);
      asm volatile("" : "+v"(sum));
      const float mean = sum / (float)C;
      float ss = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float dlt = v[ks][e][r] - mean;
            ss += dlt * dlt;
          }
      ss += __shfl_xor(ss, 16, 64);
      asm volatile("" : "+v"(ss));
      ss += __shfl_xor(ss, 32, 64);
      asm volatile("" : "+v"(ss));
      const float rstd = rsqrtf(ss / (float)C + p.ln_eps);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        half_t y[8];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const f32x4 g4 = first_read(*(const f32x4*)(p.ln_gamma + 32 * ks + 8 * fg + 4 * e));
          const f32x4 b4 = first_read(*(const f32x4*)(p.ln_beta + 32 * ks + 8 * fg + 4 * e));
#pragma unroll
          for (int r = 0; r < 4; ++r) y[4 * e + r] = (half_t)((v[ks][e][r] - mean) * rstd * g4[r] + b4[r]);
        }
        areg[i][ks] = half8_t{y[0], y[1], y[2], y[3], y[4], y[5], y[6], y[7]};
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int64_t m = m0 + 16 * i + fr;
      if (m >= p.M) m = p.M - 1;
      const half_t* ap = p.a + m * p.lda + 8 * fg;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) areg[i][ks] = *(const half8_t*)(ap + 32 * ks);
    }
  }
  f32x4 acc2[2][NJH];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int64_t m = m0 + 16 * i + fr;
    if (m >= p.M) m = p.M - 1;
#pragma unroll
    for (int jj = 0; jj < NJH; ++jj)
      acc2[i][jj] = p.residual ? *(const f32x4*)(p.residual + m * p.ldr + 16 * (h * NJH + jj) + 4 * fg) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int i = threadIdx.x; i < 2 * C; i += 512) *(f32x4*)(lds_b1 + 4 * i) = *(const f32x4*)(p.b1 + 4 * i);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(areg[i][ks]));
#pragma unroll
    for (int jj = 0; jj < NJH; ++jj) asm volatile("" : "+v"(acc2[i][jj]));
  }

  // (W1: gemm_tile.h's paired key and WRowMap<4, true>, W2: the natural key; written out in both kernels: the helpers change 1 - 3 of 8 instantiations)
  auto w1_key = [](int row) { return ((row >> 1) & 1) | (((row >> 3) & 3) << 1); };
  const half_t* w1_src[2];  // W1 tile: wave w stages rows 16w .. 16w+15 (2 passes)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wave * 16 + 8 * i + sr;
    w1_src[i] = p.w1 + (int64_t)row * C + (sp ^ w1_key(row)) * 8;
  }
  const half_t* w2_src[2];  // W2 slice: wave w stages rows (C/8)w .. ; passes two apart share the swizzle key
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wave * (C / 8) + 8 * i + sr;
    w2_src[i] = p.w2 + (int64_t)row * (4 * C) + (sp ^ ((row >> 1) & 7)) * 8;
  }
  auto stage_w1 = [&](int buf, int hc, int kt) {
    const unsigned dst = lds_base_u32 + buf * W1_BYTES + wave * 16 * 128;
    const int64_t off = (int64_t)hc * 128 * C + kt * 64;
#pragma unroll
    for (int i = 0; i < 2; ++i) glds16_raw(w1_src[i] + off, dst + i * 1024);
  };
  auto stage_w2_part = [&](int buf, int hc, int part) {
    const unsigned dst = lds_base_u32 + W1_RING * W1_BYTES + buf * W2_BYTES + wave * (C / 8) * 128;
#pragma unroll
    for (int u = 0; u < W2_PER_KT; ++u) {
      const int i = part * W2_PER_KT + u;
      if (i < W2_PASSES) glds16_raw(w2_src[i & 1] + (int64_t)(i >> 1) * 16 * (4 * C) + hc * 64, dst + i * 1024);
    }
  };

  int w1_off[2], w2_off[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int rb = 64 * h + 8 * (fr >> 2) + (fr & 3);  // this half's GEGLU group: tile rows 64h ..
    w1_off[s] = rb * 128 + (((4 * s + fg) ^ w1_key(rb)) << 4);
    const int r2 = 16 * (h * NJH) + fr;
    w2_off[s] = r2 * 128 + (((4 * s + fg) ^ ((r2 >> 1) & 7)) << 4);
  }
  char* const x_mine = lds_x + ((mr * 2 + h) * 2) * 1024 + lane * 16;
  const char* const x_q0 = lds_x + (mr * 2 * 2) * 1024 + lane * 16;  // half 0's two fragments, then half 1's

  constexpr int NTILES = NCH * NK1;
  auto stage_w1_seq = [&](int g) { stage_w1(g % W1_RING, g / NK1, g % NK1); };
  auto wait_all_but = [&](int n) {  // wave-uniform count of the loads this wave issued during the current K-tile
    if (n >= 3) wait_vm<3>();
    else if (n == 2) wait_vm<2>();
    else if (n == 1) wait_vm<1>();
    else wait_vm<0>();
  };
  __syncthreads();
  stage_w1_seq(0);
#pragma unroll
  for (int part = 0; part < NK1; ++part) stage_w2_part(0, 0, part);
  if (NTILES > 1) stage_w1_seq(1);
  if (NTILES > 1) wait_vm<2>();  // tile 0 and the first W2 slice have landed; tile 1 (2 loads) flies on
  else wait_vm<0>();
  lds_barrier();

  int g = 0;  // W1 tile sequence number
  for (int hc = 0; hc < NCH; ++hc) {
    // stage-1 accumulators start from the bias (blocks 0,1 = value e = 0,1; blocks 2,3 = gate): no bias registers or adds later
    f32x4 acc1[2][4];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float* bp = lds_b1 + hc * 128 + 64 * h + 8 * fg + 4 * e;
      acc1[0][e] = acc1[1][e] = *(const f32x4*)bp;
      acc1[0][2 + e] = acc1[1][2 + e] = *(const f32x4*)(bp + 32);
    }
#pragma unroll
    for (int kt = 0; kt < NK1; ++kt) {
      int issued = 0;
      if (g + 2 < NTILES) {
        stage_w1_seq(g + 2);
        issued += 2;
      }
      if (hc + 1 < NCH && kt * W2_PER_KT < W2_PASSES) {
        stage_w2_part((hc + 1) & 1, hc + 1, kt);
        issued += (kt + 1) * W2_PER_KT <= W2_PASSES ? W2_PER_KT : W2_PASSES - kt * W2_PER_KT;
      }
      const char* const tb = lds_w1 + (g % W1_RING) * W1_BYTES;
      half8_t bfr[2][4];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[s][j] = *(const half8_t*)(tb + w1_off[s] + (32 * (j >> 1) + 4 * (j & 1)) * 128);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bfr[s][j], areg[i][2 * kt + s], acc1[i][j], 0, 0, 0);
      wait_all_but(issued);  // tile g + 1 (issued a K-tile ago) has landed; this K-tile's loads stay in flight
      lds_barrier();
      ++g;
    }
    // GEGLU of this wave's 32 hidden features (group q = h of the chunk), handed to the partner through LDS
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f32x4 o0 = geglu4(acc1[i][0], acc1[i][2]);
      const f32x4 o1 = geglu4(acc1[i][1], acc1[i][3]);
      *(half8_t*)(x_mine + i * 1024) = half8_t{(half_t)o0[0], (half_t)o0[1], (half_t)o0[2], (half_t)o0[3],
                                               (half_t)o1[0], (half_t)o1[1], (half_t)o1[2], (half_t)o1[3]};
    }
    lds_barrier();  // both halves of every row group have published their 32 features
    half8_t hq[2][2];  // [k-step q = half that produced the features][token block i], both read back from LDS
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int i = 0; i < 2; ++i) hq[q][i] = *(const half8_t*)(x_q0 + (q * 2 + i) * 1024);
    // stage 2: this wave's half of the output blocks, k-step q = 0 / 1 <- hidden features of half 0 / 1
    const char* const t2 = lds_w2 + (hc & 1) * W2_BYTES;
#pragma unroll
    for (int jj = 0; jj < NJH; ++jj) {
      const half8_t w0 = *(const half8_t*)(t2 + w2_off[0] + jj * (16 * 128));
      const half8_t w1f = *(const half8_t*)(t2 + w2_off[1] + jj * (16 * 128));
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        acc2[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, hq[0][i], acc2[i][jj], 0, 0, 0);
        acc2[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1f, hq[1][i], acc2[i][jj], 0, 0, 0);
      }
    }
    lds_barrier();  // W2 buffer (hc & 1) and the exchange slots are rewritten during the next chunk
  }

#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t m = m0 + 16 * i + fr;
    const bool ok = m < p.M;
#pragma unroll
    for (int jj = 0; jj < NJH; ++jj) {
      const int f = 16 * (h * NJH + jj) + 4 * fg;
      const f32x4 v = acc2[i][jj] + first_read(*(const f32x4*)(p.b2 + f));
      if (!ok) continue;
      if (p.out_f32) *(f32x4*)(p.out_f32 + m * p.ldo32 + f) = v;
      if (p.out_f16) *(half4_t*)(p.out_f16 + m * p.ldo16 + f) = to_f16x4(v);
    }
  }
}


// ---------------------------------------------------------------------------------------------------------------
// e4m3 sibling of ff_fused8_kernel (seva_ff_fused_fp8, the fp8 mode's `ff="fp8"` option): the same 128-row tile, 8 waves,
// 3-deep W1 LDS-DMA ring and double-buffered W2 slice, with both GEMMs on v_mfma_scale_f32_16x16x128_f8f6f4.
//   * A: the LayerNorm prologue rounds the normalised row once to e4m3 (saturating RNE, unit scale) and zero-pads it to
//     KP = the multiple of 128 at or above C IN REGISTERS (C = 320: the sixth 64-wide chunk is zero); or e4m3 bytes `a`.
//     Registers: 2 token blocks x KP/128 K-tiles x 8 dwords (48 at C = 320, against 80 for the f16 panel).
//   * stage 1: a K-tile is 128 W1 rows x 128 bytes (128 e4m3 elements: the f16 kernel's LDS image, same swizzle); lane group
//     fg's 32-byte operand is chunks fg and 4 + fg of a row for BOTH operands (the GEMM kernels' convention).  W1 row scales
//     2^e enter as the E8M0 scale of the weight operand (constant along K); four scale bytes per chunk and lane sit in LDS.
//   * GEGLU (geglu4) -> hidden value rounded once to e4m3, 8 features (one chunk) per lane and token block.
//   * stage 2 runs once per PAIR of 64-feature chunks (one 128-deep MFMA k-step): the lane's 16 bytes of the pair plus the
//     partner wave's 16 (LDS exchange) are its B operand as they sit.  W2's columns are stored in that order (ff_fp8.h).
template <int C>
__global__ __launch_bounds__(512, 2) void ff_fused8_fp8_kernel(Ff8Args q) {
  const FfArgs& p = q.f;
  constexpr int KP = FF8_KP(C), NK1 = KP / 128, NU = C / 64;  // K-tiles of stage 1; 64-wide input chunks that hold data
  constexpr int NJ2 = C / 16, NJH = NJ2 / 2, NCH = C / 16, NP = NCH / 2, NSC2 = (NJH + 3) / 4;
  constexpr int W1_BYTES = 128 * 128, W2_BYTES = C * 128;
  constexpr int W2_PASSES = C / 64;  // 8-row passes per wave and slice (C/8 rows per wave)
  constexpr int W2_PER_KT = (W2_PASSES + 2 * NK1 - 1) / (2 * NK1);  // a slice is staged over the 2 NK1 K-tiles of a chunk pair
  static_assert(NJ2 % 2 == 0 && NCH % 2 == 0, "output blocks split over two waves; chunks taken in pairs");
  static_assert(2 + W2_PER_KT <= 3, "wait_all_but counts at most 3 loads per K-tile");
  typedef int v4i_t __attribute__((ext_vector_type(4)));

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // [W1 ring: 3 tiles][W2 buf0][W2 buf1][b1: 8C floats][W1 scale words: NCH x 2 halves x 16 rows][exchange: 16 KiB]
  constexpr int W1_RING = 3;
  char* const lds_w1 = smem;
  char* const lds_w2 = smem + W1_RING * W1_BYTES;
  float* const lds_b1 = (float*)(smem + W1_RING * W1_BYTES + 2 * W2_BYTES);
  int* const lds_s1 = (int*)(smem + W1_RING * W1_BYTES + 2 * W2_BYTES + 8 * C * 4);
  char* const lds_x = smem + W1_RING * W1_BYTES + 2 * W2_BYTES + 8 * C * 4 + NCH * 32 * 4;
  const unsigned lds_base_u32 = __builtin_amdgcn_readfirstlane(lds_addr_u32(smem));

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int mr = wave & 3, h = wave >> 2;
  const int fr = lane & 15, fg = lane >> 4;
  const int sr = lane >> 3, sp = lane & 7;

  const int tm = xcd_remap(blockIdx.x, p.tiles_m);
  const int64_t m0 = (int64_t)tm * 128 + mr * 32;

  // areg[i][u]: input elements 64 u + 16 fg .. + 15 of token row m0 + 16 i + fr; K-tile kt = lo u = 2 kt, hi u = 2 kt + 1
  half8_t areg[2][2 * NK1];
  if (p.ln_x) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int64_t m = m0 + 16 * i + fr;
      if (m >= p.M) m = p.M - 1;
      const float* xr = p.ln_x + m * p.ldx + 16 * fg;
      f32x4 v[NU][4];
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[u][e] = first_read(*(const f32x4*)(xr + 64 * u + 4 * e));
      float sum = 0.f;
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) sum += v[u][e][0] + v[u][e][1] + v[u][e][2] + v[u][e][3];
      sum += __shfl_xor(sum, 16, 64);
      asm volatile("" : "+v"(sum));
      sum += __shfl_xor(sum, 32, 64);
      asm volatile("" : "+v"(sum));
      const float mean = sum / (float)C;
      float ss = 0.f;
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float dlt = v[u][e][r] - mean;
            ss += dlt * dlt;
          }
      ss += __shfl_xor(ss, 16, 64);
      asm volatile("" : "+v"(ss));
      ss += __shfl_xor(ss, 32, 64);
      asm volatile("" : "+v"(ss));
      const float rstd = rsqrtf(ss / (float)C + p.ln_eps);
#pragma unroll
      for (int u = 0; u < 2 * NK1; ++u) {
        if (u >= NU) {  // zero padding C .. KP - 1 (W1's columns there are zero too)
          areg[i][u] = half8_t{};
          continue;
        }
        v4i_t w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const f32x4 g4 = first_read(*(const f32x4*)(p.ln_gamma + 64 * u + 16 * fg + 4 * e));
          const f32x4 b4 = first_read(*(const f32x4*)(p.ln_beta + 64 * u + 16 * fg + 4 * e));
          float y[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) y[r] = (v[u][e][r] - mean) * rstd * g4[r] + b4[r];
          w[e] = pack_fp8x4(y[0], y[1], y[2], y[3]);
        }
        areg[i][u] = __builtin_bit_cast(half8_t, w);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int64_t m = m0 + 16 * i + fr;
      if (m >= p.M) m = p.M - 1;
      const uint8_t* ap = (const uint8_t*)p.a + m * p.lda + 16 * fg;
#pragma unroll
      for (int u = 0; u < 2 * NK1; ++u) areg[i][u] = u < NU ? *(const half8_t*)(ap + 64 * u) : half8_t{};
    }
  }
  // stage-2 accumulators start from zero; the residual is added in the epilogue (loaded here, its 80 registers at C = 320 pushed
  // A fragments into scratch)
  f32x4 acc2[2][NJH];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jj = 0; jj < NJH; ++jj) acc2[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < 2 * C; i += 512) *(f32x4*)(lds_b1 + 4 * i) = *(const f32x4*)(p.b1 + 4 * i);
  // W1 scale word of (chunk hc, half hh, MFMA row f): byte j = 127 + e of the row that block j (value e0, value e1, gate e0,
  // gate e1) reads in MFMA row f -- the rows of the f16 kernel's fragment reads
  for (int idx = threadIdx.x; idx < NCH * 32; idx += 512) {
    const int hc = idx >> 5, hh = (idx >> 4) & 1, f = idx & 15;
    const int rb = hc * 128 + 64 * hh + 8 * (f >> 2) + (f & 3);
    lds_s1[idx] = (int)q.w1_exp[rb] | ((int)q.w1_exp[rb + 4] << 8) | ((int)q.w1_exp[rb + 32] << 16) | ((int)q.w1_exp[rb + 36] << 24);
  }
  // W2 row scales of this wave's output blocks (constant over the whole kernel): 4 blocks per word
  int wsc2[NSC2];
#pragma unroll
  for (int w = 0; w < NSC2; ++w) wsc2[w] = 0;
#pragma unroll
  for (int jj = 0; jj < NJH; ++jj) wsc2[jj >> 2] |= (int)q.w2_exp[16 * (h * NJH + jj) + fr] << (8 * (jj & 3));
  // retire every compiler-visible global load here: the main loop's waits are the counted ones below
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int u = 0; u < NU; ++u) asm volatile("" : "+v"(areg[i][u]));  // (the zero padding stays a constant the allocator can rematerialise)
#pragma unroll
    for (int jj = 0; jj < NJH; ++jj) asm volatile("" : "+v"(acc2[i][jj]));
  }
#pragma unroll
  for (int w = 0; w < NSC2; ++w) asm volatile("" : "+v"(wsc2[w]));

  auto w1_key = [](int row) { return ((row >> 1) & 1) | (((row >> 3) & 3) << 1); };
  unsigned w1_voff[2];  // W1 tile: wave w stages rows 16w .. 16w+15 (2 passes); byte offsets (W1 < 4 GiB)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wave * 16 + 8 * i + sr;
    w1_voff[i] = (unsigned)(row * KP + (sp ^ w1_key(row)) * 16);
  }
  unsigned w2_voff[2];  // W2 slice: wave w stages rows (C/8)w .. ; passes two apart share the swizzle key
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wave * (C / 8) + 8 * i + sr;
    w2_voff[i] = (unsigned)(row * (4 * C) + (sp ^ ((row >> 1) & 7)) * 16);
  }
  auto stage_w1 = [&](int buf, int hc, int kt) {
    const unsigned dst = lds_base_u32 + buf * W1_BYTES + wave * 16 * 128;
    const uint8_t* const base = (const uint8_t*)p.w1 + (int64_t)hc * 128 * KP + kt * 128;
#pragma unroll
    for (int i = 0; i < 2; ++i) glds16_sv(base, w1_voff[i], dst + i * 1024);
  };
  auto stage_w2_part = [&](int buf, int pp, int part) {
    const unsigned dst = lds_base_u32 + W1_RING * W1_BYTES + buf * W2_BYTES + wave * (C / 8) * 128;
#pragma unroll
    for (int u = 0; u < W2_PER_KT; ++u) {
      const int i = part * W2_PER_KT + u;
      if (i < W2_PASSES)
        glds16_sv((const uint8_t*)p.w2 + (int64_t)(i >> 1) * 16 * (4 * C) + pp * 128, w2_voff[i & 1], dst + i * 1024);
    }
  };

  int w1_off[2], w2_off[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int rb = 64 * h + 8 * (fr >> 2) + (fr & 3);
    w1_off[s] = rb * 128 + (((4 * s + fg) ^ w1_key(rb)) << 4);
    const int r2 = 16 * (h * NJH) + fr;
    w2_off[s] = r2 * 128 + (((4 * s + fg) ^ ((r2 >> 1) & 7)) << 4);
  }
  char* const x_mine = lds_x + ((mr * 2 + h) * 2) * 1024 + lane * 16;
  const char* const x_q0 = lds_x + (mr * 2 * 2) * 1024 + lane * 16;  // half 0's two fragments, then half 1's

  constexpr int NTILES = NCH * NK1;
  auto stage_w1_seq = [&](int g) { stage_w1(g % W1_RING, g / NK1, g % NK1); };
  auto wait_all_but = [&](int n) {
    if (n >= 3) wait_vm<3>();
    else if (n == 2) wait_vm<2>();
    else if (n == 1) wait_vm<1>();
    else wait_vm<0>();
  };
  __syncthreads();
  stage_w1_seq(0);
#pragma unroll
  for (int part = 0; part < 2 * NK1; ++part) stage_w2_part(0, 0, part);
  stage_w1_seq(1);
  wait_vm<2>();  // tile 0 and the first W2 slice have landed; tile 1 (2 loads) flies on
  lds_barrier();

  int g = 0;  // W1 tile sequence number
  for (int pp = 0; pp < NP; ++pp) {
    v4i_t hx[2];  // [token block]: e4m3 hidden features of chunk 2 pp (bytes 0..7) and 2 pp + 1 (bytes 8..15)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int hc = 2 * pp + c;
      // stage-1 accumulators start from zero, b1 is added after the chunk's last K-tile: no bias registers live under the MFMAs
      f32x4 acc1[2][4];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc1[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int sc1 = lds_s1[hc * 32 + h * 16 + fr];
#pragma unroll
      for (int kt = 0; kt < NK1; ++kt) {
        int issued = 0;
        if (g + 2 < NTILES) {
          stage_w1_seq(g + 2);
          issued += 2;
        }
        const int kk = c * NK1 + kt;
        if (pp + 1 < NP && kk * W2_PER_KT < W2_PASSES) {
          stage_w2_part((pp + 1) & 1, pp + 1, kk);
          issued += (kk + 1) * W2_PER_KT <= W2_PASSES ? W2_PER_KT : W2_PASSES - kk * W2_PER_KT;
        }
        const char* const tb = lds_w1 + (g % W1_RING) * W1_BYTES;
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {  // value blocks, then gate blocks: 16 fragment registers live, not 32
          half8_t bfr[2][2];
#pragma unroll
          for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int e = 0; e < 2; ++e) bfr[s][e] = *(const half8_t*)(tb + w1_off[s] + (32 * jp + 4 * e) * 128);
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 2; ++e)
              acc1[i][2 * jp + e] = mfma_f8(2 * jp + e, bfr[0][e], bfr[1][e], areg[i][2 * kt], areg[i][2 * kt + 1], acc1[i][2 * jp + e], sc1);
          if (jp == 0) __builtin_amdgcn_sched_barrier(0);
        }
        // the K-tile's scaled MFMAs stay in front of its barrier (gemm.hip / conv_win.hip: hipcc otherwise sinks them behind it)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(acc1[i][j]));
        wait_all_but(issued);  // tile g + 1 (issued a K-tile ago) has landed; this K-tile's loads stay in flight
        lds_barrier();
        ++g;
      }
      f32x4 bias[4];  // blocks 0, 1 = value e = 0, 1; blocks 2, 3 = gate
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float* bp = lds_b1 + hc * 128 + 64 * h + 8 * fg + 4 * e;
        bias[e] = first_read(*(const f32x4*)bp);
        bias[2 + e] = first_read(*(const f32x4*)(bp + 32));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f32x4 o0 = geglu4(acc1[i][0] + bias[0], acc1[i][2] + bias[2]);
        const f32x4 o1 = geglu4(acc1[i][1] + bias[1], acc1[i][3] + bias[3]);
        hx[i][2 * c] = pack_fp8x4(o0[0], o0[1], o0[2], o0[3]);
        hx[i][2 * c + 1] = pack_fp8x4(o1[0], o1[1], o1[2], o1[3]);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) *(v4i_t*)(x_mine + i * 1024) = hx[i];
    lds_barrier();  // both halves of every row group have published the pair's features
    half8_t hq[2][2];  // [half q that produced the features = lo / hi 16 bytes of the operand][token block i]
#pragma unroll
    for (int qq = 0; qq < 2; ++qq)
#pragma unroll
      for (int i = 0; i < 2; ++i) hq[qq][i] = *(const half8_t*)(x_q0 + (qq * 2 + i) * 1024);
    const char* const t2 = lds_w2 + (pp & 1) * W2_BYTES;
#pragma unroll
    for (int jj = 0; jj < NJH; ++jj) {
      const half8_t w0 = *(const half8_t*)(t2 + w2_off[0] + jj * (16 * 128));
      const half8_t w1f = *(const half8_t*)(t2 + w2_off[1] + jj * (16 * 128));
#pragma unroll
      for (int i = 0; i < 2; ++i) acc2[i][jj] = mfma_f8(jj, w0, w1f, hq[0][i], hq[1][i], acc2[i][jj], wsc2[jj >> 2]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < NJH; ++jj) asm volatile("" : "+v"(acc2[i][jj]));
    lds_barrier();  // W2 buffer (pp & 1) and the exchange slots are rewritten during the next pair
  }

#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t m = m0 + 16 * i + fr;
    const bool ok = m < p.M;
#pragma unroll
    for (int jj = 0; jj < NJH; ++jj) {
      const int f = 16 * (h * NJH + jj) + 4 * fg;
      if (!ok) continue;
      f32x4 v = acc2[i][jj] + first_read(*(const f32x4*)(p.b2 + f));
      if (p.residual) v += first_read(*(const f32x4*)(p.residual + m * p.ldr + f));
      if (p.out_f32) *(f32x4*)(p.out_f32 + m * p.ldo32 + f) = v;
      if (p.out_f16) *(half4_t*)(p.out_f16 + m * p.ldo16 + f) = to_f16x4(v);
    }
  }
}

// ---- host side: one set of checks, one argument builder, one work account and one launcher for both entry points ----
// `pre`: "ff_fused" / "ff_fused_fp8", the prefix of every error text.  FP8: e4m3 operands (lda counts bytes; `a` is not read, so not
// checked, under the LayerNorm prologue) and the two E8M0 scale vectors.
template <bool FP8>
int validate_ff(const seva_ff_desc* d, const char* pre) {
  SEVA_REQUIRE(d != nullptr, "%s: null desc", pre);
  SEVA_REQUIRE(d->C == 64 || d->C == 128 || d->C == 256 || d->C == 320, "%s: C=%d unsupported (64, 128, 256, 320)", pre, d->C);
  if constexpr (FP8) {
    SEVA_REQUIRE(d->a || d->ln_x, "%s: neither a nor ln_x given", pre);
    SEVA_REQUIRE(d->w1 && d->b1 && d->w2 && d->b2, "%s: null operand", pre);
    SEVA_REQUIRE(d->w1_exp && d->w2_exp, "%s: w1_exp and w2_exp (per-row E8M0 scale bytes) are required", pre);
  } else {
    SEVA_REQUIRE((d->a || d->ln_x) && d->w1 && d->b1 && d->w2 && d->b2, "%s: null operand", pre);
  }
  SEVA_REQUIRE(!d->ln_x || (d->ln_gamma && d->ln_beta && d->ldx >= d->C && d->ldx % 4 == 0 &&
                            ((uintptr_t)d->ln_x | (uintptr_t)d->ln_gamma | (uintptr_t)d->ln_beta) % 16 == 0),
               "%s: LayerNorm prologue needs gamma, beta, a row pitch >= C (multiple of 4), 16-byte aligned pointers", pre);
  SEVA_REQUIRE(d->out_f32 || d->out_f16, "%s: no output", pre);
  SEVA_REQUIRE(d->M > 0, "%s: empty problem", pre);
  if constexpr (FP8) {
    SEVA_REQUIRE(d->ln_x || (d->lda >= d->C && d->lda % 16 == 0), "%s: lda=%lld invalid (bytes, >= C, multiple of 16)", pre, (long long)d->lda);
  } else {
    SEVA_REQUIRE(d->ln_x || (d->lda >= d->C && d->lda % 8 == 0), "%s: lda=%lld invalid", pre, (long long)d->lda);
  }
  SEVA_REQUIRE((!d->residual || d->ldr % 4 == 0) && (!d->out_f32 || d->ldo32 % 4 == 0) && (!d->out_f16 || d->ldo16 % 4 == 0),
               "%s: row pitches must be multiples of 4", pre);
  SEVA_REQUIRE(((uintptr_t)(FP8 && d->ln_x ? nullptr : d->a) | (uintptr_t)d->w1 | (uintptr_t)d->b1 | (uintptr_t)d->w2 | (uintptr_t)d->b2 |
                (uintptr_t)d->residual | (uintptr_t)d->out_f32 | (uintptr_t)d->out_f16) % 16 == 0,
               "%s: pointers must be 16-byte aligned", pre);
  SEVA_REQUIRE((d->M + 127) / 128 <= 0x7fffffff, "%s: too many rows", pre);
  return 0;
}

FfArgs ff_args(const seva_ff_desc* d) {
  FfArgs a{};
  a.a = (const half_t*)d->a; a.w1 = (const half_t*)d->w1; a.b1 = d->b1; a.w2 = (const half_t*)d->w2; a.b2 = d->b2;
  a.residual = d->residual; a.out_f32 = d->out_f32; a.out_f16 = (half_t*)d->out_f16;
  a.M = d->M; a.lda = d->lda; a.ldr = d->ldr; a.ldo32 = d->ldo32; a.ldo16 = d->ldo16;
  a.ln_x = d->ln_x; a.ln_gamma = d->ln_gamma; a.ln_beta = d->ln_beta; a.ldx = d->ldx; a.ln_eps = d->ln_eps;
  a.tiles_m = (int)((d->M + 127) / 128);
  return a;
}

// algorithmic FLOP and HBM bytes: rows read (fp32 under the LayerNorm prologue, else a_bytes per element) and written once, weights once
struct FfWork { double flops, bytes; };
FfWork ff_work(const seva_ff_desc* d, double a_bytes, double w_bytes) {
  const double C = (double)d->C, M = (double)d->M;
  return {2.0 * M * C * (8.0 * C) + 2.0 * M * (4.0 * C) * C,
          M * C * ((d->ln_x ? 4.0 : a_bytes) + (d->residual ? 4.0 : 0.0) + (d->out_f32 ? 4.0 : 0.0) + (d->out_f16 ? 2.0 : 0.0)) + w_bytes};
}

template <class Args>
int ff_launch(void (*kernel)(Args), const char* name, int lds, std::atomic<uint64_t>& attr_devs, const Args& a, int tiles_m, hipStream_t s) {
  seva_max_dynamic_lds_once(attr_devs, lds, {(const void*)kernel});
  hipLaunchKernelGGL(kernel, dim3((unsigned)tiles_m), dim3(512), lds, s, a);
  return seva_check_launch(name);
}
template <int C>
int ff_launch8(const FfArgs& a, hipStream_t s) {
  static std::atomic<uint64_t> attr_devs{0};
  return ff_launch(ff_fused8_kernel<C>, "ff_fused8_kernel", 3 * 128 * 128 + 2 * C * 128 + 8 * C * 4 + 16 * 1024, attr_devs, a, a.tiles_m, s);
}
template <int C>
int ff_launch8_fp8(const Ff8Args& a, hipStream_t s) {
  constexpr int lds = 3 * 128 * 128 + 2 * C * 128 + 8 * C * 4 + (C / 16) * 32 * 4 + 16 * 1024;
  static_assert(lds <= 160 * 1024, "LDS budget of one workgroup per CU");
  static std::atomic<uint64_t> attr_devs{0};
  return ff_launch(ff_fused8_fp8_kernel<C>, "ff_fused8_fp8_kernel", lds, attr_devs, a, a.f.tiles_m, s);
}

}  // namespace

extern "C" int seva_ff_fused_f16(const seva_ff_desc* d, seva_stream_t stream) {
  if (const int rc = validate_ff<false>(d, "ff_fused")) return rc;
  const FfArgs a = ff_args(d);
  hipStream_t s = (hipStream_t)stream;
  const double C = (double)d->C;
  const FfWork w = ff_work(d, 2.0, 2.0 * (8.0 * C * C + 4.0 * C * C));
  SevaProfScope prof(0, w.flops, s, w.bytes);
  switch (d->C) {
    case 64: return ff_launch8<64>(a, s);
    case 128: return ff_launch8<128>(a, s);
    case 256: return ff_launch8<256>(a, s);
    default: return ff_launch8<320>(a, s);
  }
}

// e4m3 operands (ff_fp8.h): a [M][lda] bytes (columns C .. KP - 1 are not read) or the LayerNorm prologue; w1 [8C][KP], w2 [C][4C]
// column-permuted, w1_exp [8C] / w2_exp [C] E8M0 row scales.
extern "C" int seva_ff_fused_fp8(const seva_ff_desc* d, seva_stream_t stream) {
  if (const int rc = validate_ff<true>(d, "ff_fused_fp8")) return rc;
  Ff8Args a{ff_args(d), (const uint8_t*)d->w1_exp, (const uint8_t*)d->w2_exp};
  hipStream_t s = (hipStream_t)stream;
  const double C = (double)d->C;
  const FfWork w = ff_work(d, 1.0, 8.0 * C * FF8_KP(d->C) + 4.0 * C * C);
  SevaProfScope prof(0, w.flops, s, w.bytes);
  switch (d->C) {
    case 64: return ff_launch8_fp8<64>(a, s);
    case 128: return ff_launch8_fp8<128>(a, s);
    case 256: return ff_launch8_fp8<256>(a, s);
    default: return ff_launch8_fp8<320>(a, s);
  }
}
