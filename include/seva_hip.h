/* seva_hip.h -- C-ABI of libseva_hip.so: the MI355X (gfx950) kernels behind the
 * `seva.model` / `seva.sampling` operator API of Stable Virtual Camera.
 *
 * The reference (atakan-topaloglu/stable-virtual-camera) has no FFI layer: below its Python
 * operator API sit PyTorch ATen ops.  This library sits exactly there.
 * Each entry point names the reference lines whose arithmetic it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless stated; no allocation, no ownership transfer;
 *  - `seva_stream_t` is a hipStream_t; all work is enqueued on it, nothing synchronises;
 *  - return 0 on success, a negative code on error; `seva_last_error()` gives the message
 *    (thread-local);
 *  - activations are channels-last: a (n, c, h, w) tensor of the reference is stored as
 *    [n][h*w][c]; "f16" is IEEE binary16, "f32" binary32;
 *  - all entry points are graph-capture safe (no sync, no malloc).
 */
#ifndef SEVA_HIP_H
#define SEVA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* seva_stream_t;

#define SEVA_OK 0
#define SEVA_ERR_ARG (-1)
#define SEVA_ERR_LAUNCH (-2)
#define SEVA_ERR_UNSUPPORTED (-3)

const char* seva_last_error(void);
/* Name of the instantiation-table row (csrc/gemm_plan.h: SEVA_GEMM_KERNELS / SEVA_WIN_KERNELS) of the last seva_gemm_f16 /
 * seva_gemm_f16_split_out / seva_gemm_fp8 launch the calling thread planned; "" before any.  Thread-local, host only, a static
 * string (never freed).  A call that failed before a row was chosen leaves the previous name.  (No ABI change: a new symbol only.) */
const char* seva_last_plan(void);
/* ABI version of this header; bumped on any signature or struct change, and on a changed VALUE of a contract constant below.
 * A new macro that names a number the contract already had is not an ABI change (nor is a new symbol).
 *
 * Contract constants: every number that both sides of this ABI must agree on -- a caller needs it to size a buffer or to predict
 * which path a launch takes -- is a SEVA_* macro of this header, used under that name by the kernels' host code and restated once on
 * the Python side (seva/ops.py, seva/_native.py); tests/test_abi_cpu.py compares the two.  Tuning numbers that only the kernels know
 * are not here. */
#define SEVA_ABI_VERSION 12
int seva_abi_version(void);
/* Name of the code object's target, e.g. "gfx950". */
const char* seva_target_arch(void);

/* ------------------------------------------------------------------------------------------
 * GEMM / implicit-GEMM 3x3 convolution on fp16 MFMA with fp32 accumulation.
 *   out[m][n] = sum_k A[m][k] * W[n][k]  (+ bias[n]) (+ row_add[m / rows_per_group][n])   [row pitch ld_row_add]
 *                                        (+ residual[m][n])
 * Replaces nn.Linear (seva/modules/transformer.py:11,30,52-57,187,200), nn.Conv2d 1x1/3x3
 * (seva/modules/layers.py:40,55,101,106-108,113,118; seva/model.py:57,173), the nearest-2x
 * upsample feeding a conv (layers.py:43-45), the GEGLU gate (transformer.py:13-15) and the
 * residual / timestep-embedding adds fused into them (layers.py:133-138, transformer.py:107-109).
 *
 * mode 0 (plain): A is [M][lda] f16.
 * mode 1 (conv3x3, pad 1): A is an NHWC f16 image [n][ih][iw][cin]; K = 9*cin ordered
 *   (ky, kx, ci); M = n*oh*ow.  `stride` is 1 or 2.  `upsample`=1 applies the conv to the
 *   nearest-neighbour 2x upsampling of A without materialising it (oh = 2*ih).
 *   `upsample`=2 (seva_gemm_f16 only) is the same operator PHASE-DECOMPOSED: after a nearest-2x upsample, output rows 2i and
 *   2i + 1 read source rows {i-1, i, i} and {i, i, i+1} (columns alike), so every output phase (py, px) is a 2x2 conv on the
 *   source image with tap (a, b) at source offset (a + py - 1, b + px - 1): 4 taps instead of 9.  `w` is then f16
 *   [4 phases 2*py+px][N][4*cin], K ordered (a, b, ci), each entry the sum of the 3x3 weights that meet on that source
 *   pixel (py = 0: a = 0 <- W[0], a = 1 <- W[1] + W[2]; py = 1: a = 0 <- W[0] + W[1], a = 1 <- W[2]; columns alike), summed
 *   by the caller BEFORE the one rounding to f16.  K = 4*cin per phase, oh = 2*ih, ow = 2*iw, M = n*oh*ow; output row of
 *   source pixel (i, j) of image g and phase (py, px): g*oh*ow + (2i + py)*ow + 2j + px.  Runs on the window-staged kernel
 *   only, with bias + out_f32 and nothing else: residual, row_add, out_f16, out_f8, a2, splitk_ws, ch_stats, col_scale,
 *   seva_gemm_fp8, N % 160 != 0, or an image whose tiles do not fit the window (or conv_win knob 0) are an ERROR, never a
 *   fall-back -- no other kernel reads this weight layout.  alg_K may be 9*cin (the reference-equivalent reduction).  The
 *   result differs from `upsample`=1 by one f16 weight rounding (two draws of the same noise).  No new symbol and no change
 *   to the struct: the ABI version is unchanged.
 *   `upsample`=4 (seva_gemm_f16 only) is value 2 on the 128-column tiles, for the VAE decoders' upsample convs (128 / 256 / 512
 *   channels, source rows up to 288 pixels): the same `w` [4][N][4*cin], K = 4*cin, oh = 2*ih, ow = 2*iw and output rows, with
 *   N % 128 == 0 and cin % 64 == 0, and bias + out_f32 + optional ch_stats.  Tiles are consecutive source pixels where one
 *   image's window fits, else 16 source columns x 8 source rows (iw % 16 == 0 and ih % 8 == 0); which is decided from one
 *   image's dimensions.  ch_stats needs ih*iw % 64 == 0 (else an ERROR; 64 = SEVA_CH_STATS_ROWS): a block is then 64 source pixels of ONE phase, i.e.
 *   64 output pixels of one image, stored as block 4*(source block) + 2*py + px, so that the oh*ow/64 blocks of image i are
 *   exactly [i*oh*ow/64, (i+1)*oh*ow/64), each written once; consumers rely only on the blocks of an image adding up to that
 *   image.  residual, row_add, out_f16, out_f8, a2, splitk_ws, col_scale, GEGLU, seva_gemm_fp8, a shape neither tiling
 *   takes, or conv_win knob 0 are an ERROR, never a fall-back.  Values 2 and 3 are unchanged (3 is an error); no new symbol,
 *   no change to the struct, the ABI version is unchanged.
 * epilogue 0: linear.  epilogue 1 (GEGLU): W rows are interleaved in groups of 64 as
 *   [32 value rows | 32 gate rows] (same for bias); output has N/2 columns:
 *   out[m][f] = (v + bv) * gelu_erf(g + bg).
 * Requirements: K % 64 == 0, cin % 64 == 0 (mode 1), N % 4 == 0, all row pitches % 4 == 0,
 * pointers 16-byte aligned.
 */
#define SEVA_CH_STATS_ROWS 64        /* output rows per block of seva_gemm_desc.ch_stats */
#define SEVA_SPLITK_FLAGS 16384      /* int flags at the head of seva_gemm_desc.splitk_ws */
#define SEVA_SPLITK_ERROR_SLOT 16383 /* the last of them counts consumers that gave up waiting: a launch has fewer tiles than this */
#define SEVA_SPLITK_TILE_M 128       /* rows and */
#define SEVA_SPLITK_TILE_N 160       /*   largest column count of one split-K tile's fp32 slot in the workspace */
#define SEVA_SPLITK_MAX_PIXELS 128   /* output pixels per sample up to which a convolution qualifies for the split */
typedef struct seva_gemm_desc {
  const void* a;
  const void* w;         /* f16 [N][K] */
  const float* bias;     /* [N] or NULL */
  const float* row_add;  /* [ceil(M / rows_per_group)][ld_row_add] or NULL */
  const float* residual; /* [M][ldr] or NULL */
  float* out_f32;        /* [M][ldo32] or NULL */
  void* out_f16;         /* [M][ldo16] or NULL */
  int64_t M, N, K;
  int64_t lda, ldr, ldo32, ldo16;
  int64_t rows_per_group;
  int64_t ld_row_add;    /* row pitch of row_add (>= N; 0 means N) */
  int32_t mode;
  int32_t epilogue;
  int32_t n, ih, iw, cin, oh, ow, stride, upsample;
  /* out[:, f] = (a @ w^T + bias)[:, f] * col_scale for f < col_scale_n (fp32, before the f16
   * rounding); 0 columns = off.  Mode 0 only, plain epilogue without residual / row_add.  Used to fold the
   * softmax scale * log2(e) into the q third of a fused QKV projection.  A convolution (mode 1) with
   * col_scale_n > 0 is an ERROR: it used to be applied by the per-tap kernel and ignored by the window kernel. */
  float col_scale;
  int32_t col_scale_n;
  /* conv mode: 1 = zero padding only at the bottom / right edge (taps start AT pixel (stride*oy, stride*ox)); the
   * stride-2 Downsample2D of the diffusers VAE encoder pads (0,1,0,1).  0 = symmetric pad 1 (every UNet conv). */
  int32_t pad_br_only;
  /* seva_gemm_fp8 only (NULL / 0 for seva_gemm_f16).  EVERY e4m3 output of this library ("saturating" below) is one round-to-nearest-even
   * of the fp32 value: finite and infinite values saturate at +-448, NaN stays NaN (byte 0x7F or 0xFF), as torch's float8_e4m3fn cast
   * of the value clamped to +-448 (tests/test_output_rounding_gpu.py). */
  const void* w_exp;     /* uint8 [N]: E8M0 scale byte 127 + e[n]; weight row n holds e4m3(w[n] * 2^-e[n]) */
  void* out_f8;          /* GEGLU epilogue: e4m3 [M][ldo8] (saturating, NaN kept), the next fp8 GEMM's A operand; or NULL.  ABI 10: also the
                          * plain epilogue of a 3x3 convolution of seva_gemm_fp8 (window kernel only): the fp32 result (bias, residual,
                          * row_add) as saturating RNE e4m3 (NaN kept), alone or beside out_f32 / out_f16, e.g. the A operand of the next fp8 conv.
                          * ldo8 and the pointer must be multiples of 8.  Not together with `upsample` (an ERROR). */
  int64_t ldo8;
  /* optional (NULL = off): GroupNorm statistics of out_f32, emitted by the epilogue while the values are in registers,
   * so that the GroupNorm consuming this tensor (seva_groupnorm_desc.stats1 / stats2) needs no statistics pass over it.
   * With R = SEVA_CH_STATS_ROWS, float [ceil(M / R)][2][N]: for every block of R output rows and every output channel, the sum
   * ([..][0][n]) and the sum of squares ([..][1][n]) of the fp32 values stored (after bias / row_add / residual); rows >= M contribute
   * nothing.  A block is R consecutive rows aligned to multiples of R rows of the whole tensor, EXCEPT for 3x3
   * convolutions over images at least 144 pixels wide with N % 160 != 0, or any such e4m3 convolution (ABI 10), or an e4m3 stride-2
   * pad_br_only convolution whose image is too wide for its linear tiles (ABI 11) (the 2-D tiles of the window-staged kernel), or a phase-decomposed upsample conv (`upsample` = 4: blocks of one output phase), where the blocks [i * hw / R, (i + 1) * hw / R) partition the pixels of image i in tile order: consumers must
   * only rely on the blocks of an image adding up to that image (seva_groupnorm does).  Per channel, so any grouping or
   * channel concatenation can be formed by the consumer.  Plain epilogue with out_f32 and N >= 128 only; forces 128-row tiles. */
  float* ch_stats;
  /* optional (NULL = off) workspace that lets seva_gemm_f16 run a convolution over small images (<= SEVA_SPLITK_MAX_PIXELS output
   * pixels per sample, K >= 1024: the 9x9 level of a 576x576 step) as split-K = 2 on 128-row tiles: two workgroups per tile, the
   * upper half of K exported raw, added by the partner before the epilogue (fixed association: deterministic, and chosen
   * from per-sample dimensions only).  Layout: SEVA_SPLITK_FLAGS int flags (zero before first use; every launch leaves them zero;
   * flag SEVA_SPLITK_ERROR_SLOT counts hand-offs that were given up, so a launch has fewer tiles than that), then one
   * SEVA_SPLITK_TILE_M x BN fp32 tile per output tile, BN <= SEVA_SPLITK_TILE_N: splitk_ws_bytes >= 4 * (SEVA_SPLITK_FLAGS +
   * tiles * SEVA_SPLITK_TILE_M * SEVA_SPLITK_TILE_N), tiles = ceil(M / SEVA_SPLITK_TILE_M) * ceil(N / BN) with BN >= 128.  The hand-off
   * uses agent-scope (sc1) stores / loads, no cache-wide fence.  One launch at a time may
   * use a given workspace (launches on ONE stream are fine).  A workspace too small for a launch that qualifies for the split is
   * an ERROR (ABI 8; it was a silent fall-back to the unsplit kernel): whether a sample is split never depends on the batch. */
  float* splitk_ws;
  int64_t splitk_ws_bytes;
  /* optional second A operand of a 3x3 convolution (ABI 7; mode 1, no upsample): a2 [M][lda2] f16 whose K2 columns (K2 % 64 == 0)
   * FOLLOW the nine taps in the reduction, K = 9 * cin + K2 and w = [w_conv | w_2] per output row.  Folds the ResBlock's 1x1
   * skip convolution (seva/modules/layers.py:137-139: `skip_connection(x) + h`) into its second 3x3 conv: one accumulation, no
   * fp32 round trip of the skip result, one launch fewer. */
  const void* a2;
  int64_t lda2;
  int64_t K2;
  /* accounting only (ABI 8; seva_prof_collect): reduction length of the REFERENCE-equivalent operator when the executed one is
   * longer -- zero-padded input channels (the stem: 11 of 64), split-precision [hi | lo] operands (K doubled).  0 = K.  The
   * profiler's FLOP count of the launch is 2 M N alg_K, so that a kernel class's achieved TFLOP/s is never credited with padding. */
  int64_t alg_K;
} seva_gemm_desc;
int seva_gemm_f16(const seva_gemm_desc* d, seva_stream_t stream);
/* The same operator in GEMM mode (mode 0) whose f16 output is a split-precision operand (no ABI change: a new symbol only):
 * out_f16 (required) is written as [hi(NO) | lo(NO)] with ldo16 >= 2 NO, NO = N (plain epilogue) or N / 2 (GEGLU): hi = f16(v),
 * lo = f16(v - f32(hi)) of the fp32 epilogue value v (after bias / row_add / residual / col_scale / GEGLU).  Columns >= 2 NO of a
 * wider row are not touched.  out_f32 may be written beside it.  Conv mode, out_f8, w_exp and ch_stats are an ERROR, never a
 * fall-back to a plain f16 output.  One tile shape per epilogue and width, whatever M. */
int seva_gemm_f16_split_out(const seva_gemm_desc* d, seva_stream_t stream);
/* BASELINE config 5 ("fp8 weights, CDNA4 fp8 MFMA"): the same operator with BOTH operands in OCP e4m3 (a: [M][lda]
 * bytes or an NHWC e4m3 image, w: [N][K] bytes) on v_mfma_scale_f32_16x16x128_f8f6f4 with fp32 accumulation; the
 * per-output-channel power-of-two weight scale enters as the MFMA's E8M0 block scale, so the accumulator holds the
 * de-quantised product and bias / row_add / residual / GEGLU / col_scale behave exactly as in seva_gemm_f16.
 * K % 128 == 0 (conv: cin % 128 == 0), N % 16 == 0.  A 3x3 conv with the fused nearest-2x upsample or with out_f8 (ABI 10; the
 * VAE decoder's fp8 mode) runs on the window-staged kernel only: stride 1, pad 1, N % 128 == 0, linear tiles where the image's
 * window fits, 2-D tiles of 16 output columns (ow % 16 == 0, oh % 8 == 0) otherwise; where that kernel declines (or the conv_win
 * knob is 0) the call is an ERROR, not a fall-back to the per-tap gather, which has neither.  ABI 11 (the VAE encoder's fp8 mode): the
 * window-staged kernel has a 3x3 / stride 2 / pad_br_only family (N % 128 == 0; linear tiles where one image's window fits, 2-D tiles of
 * 16 x 8 output pixels otherwise; no out_f8).  It measured slower than the per-tap gather on the encoder's shapes, so such a conv takes the
 * gather by default; with the conv_win knob at 1 or 2 it runs on that family, and where the family declines the call is an ERROR.
 * Stride-2 convs with symmetric padding (the UNet's) keep the gather.  The reference keeps bf16 weights
 * (seva/utils.py:50-53): this is a separate precision mode, reported separately from the f16 parity mode. */
int seva_gemm_fp8(const seva_gemm_desc* d, seva_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused GEGLU feed-forward (FeedForward of seva/modules/transformer.py:18-34) for narrow levels, C in {64,128,256,320}:
 *   out[m][:] = W2 . (v * gelu_erf(g)) + b2 (+ residual[m][:]),  [v ; g] = W1 . a[m][:] + b1
 * a: f16 [M][lda]; w1: f16 [8C][C] and b1: [8C] in the interleaved GEGLU layout of seva_gemm_f16 (groups of 64 rows =
 * [32 value | 32 gate]); w2: f16 [C][4C]; b2: [C].  The 4C-wide hidden activations stay in registers (rounded to f16
 * once, as the two-kernel form rounds the stored tensor); fp32 accumulation.  The preceding LayerNorm can be folded in.
 */
typedef struct seva_ff_desc {
  const void* a;
  const void* w1;
  const float* b1;
  const void* w2;
  const float* b2;
  const float* residual; /* [M][ldr] or NULL */
  float* out_f32;        /* [M][ldo32] or NULL */
  void* out_f16;         /* [M][ldo16] or NULL */
  int64_t M, lda, ldr, ldo32, ldo16;
  int32_t C;
  /* optional LayerNorm prologue (transformer.py:102-104,141-143: ff(norm(x))): when ln_x is set the A operand is
   * LayerNorm(ln_x) * ln_gamma + ln_beta computed in registers from fp32 rows [M][ldx] and `a` is ignored. */
  const float* ln_x;
  const float* ln_gamma;
  const float* ln_beta;
  int64_t ldx;
  float ln_eps;
  /* seva_ff_fused_fp8 only (ABI 12; ignored by seva_ff_fused_f16): uint8 E8M0 scale bytes 127 + e, one per weight row:
   * w1_exp [8C] (interleaved row order), w2_exp [C]; row n of a weight holds e4m3(w[n] * 2^-e[n]). */
  const void* w1_exp;
  const void* w2_exp;
} seva_ff_desc;
int seva_ff_fused_f16(const seva_ff_desc* d, seva_stream_t stream);
/* e4m3 sibling (ABI 12; the fp8 mode's `ff="fp8"` option): the same operator on v_mfma_scale_f32_16x16x128_f8f6f4 with fp32
 * accumulation.  a: e4m3 [M][lda] bytes (lda >= C, a multiple of 16; columns >= C are not read) or the LayerNorm prologue, whose
 * normalised row is rounded once to e4m3 (saturating, NaN kept, round-to-nearest-even, unit scale); w1: e4m3 [8C][KP] with KP = the multiple
 * of 128 at or above C and zero columns >= C, interleaved GEGLU rows as above; w2: e4m3 [C][4C] with its columns permuted into the
 * kernel's order of the hidden features (csrc/ff_fp8.h; seva.ops.pack_ff_fp8 writes both).  The hidden value v * gelu_erf(g) is
 * rounded once to e4m3 (saturating, NaN kept), the value the two-kernel e4m3 chain stores through seva_gemm_desc.out_f8.  w1_exp and w2_exp
 * are required.  Every output row depends on its own input row only. */
int seva_ff_fused_fp8(const seva_ff_desc* d, seva_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Scaled-dot-product attention, head dim 64, no mask, fp16 in/out, fp32 softmax.
 * Replaces F.scaled_dot_product_attention under sdpa_kernel(FLASH_ATTENTION)
 * (seva/modules/transformer.py:66-72) for the three regimes of SURVEY.md §2.1: per-frame,
 * joint (view*h*w) and temporal (L = num_frames, batch = pixels).  The temporal regime reads
 * the (b t) s c layout in place through strides instead of the transposes at
 * transformer.py:149,154.
 * Element (b0, b1, token l, head h, d) of q lives at q + b0*q_sb0 + b1*q_sb1 + l*q_sl + h*64 + d
 * (strides in elements); k and v share strides; out likewise.
 */
#define SEVA_ATTN_LONG_MIN_LQ 2048     /* query length from which the long-sequence kernels (attn16, seva_attention_pv8's) take over */
#define SEVA_ATTN_SPLIT_MIN_LK 6144    /* key length from which those kernels split the K/V range in two, given split_ws */
#define SEVA_ATTN_SPLIT_ROW_FLOATS 66  /* floats of split_ws per half and query row */
typedef struct seva_attn_desc {
  const void* q;
  const void* k;
  const void* v;
  void* out;
  int64_t q_sb0, q_sb1, q_sl;
  int64_t k_sb0, k_sb1, k_sl;
  int64_t o_sb0, o_sb1, o_sl;
  int32_t nb0, nb1;
  int32_t heads;
  int32_t lq, lk;
  float scale;
  /* non-zero: q already holds q * scale * log2(e) (see seva_gemm_desc.col_scale); `scale` is ignored
   * and the kernel evaluates softmax as exp2(q' . k - max) */
  int32_t q_prescaled;
  /* optional workspace (ABI 7) for the K/V split of LONG sequences: with it, launches of the long-sequence kernels (lq >=
   * SEVA_ATTN_LONG_MIN_LQ, q_prescaled) whose key length is >= SEVA_ATTN_SPLIT_MIN_LK (the joint
   * view x space attention at 36x36 / 18x18: L = 27216 / 6804) run every query block as TWO workgroups over the two halves of
   * the K/V tiles plus a small fp32 combine -- the split is a function of lk only, so a sample's result does not depend on
   * the batch.  It fills the last, partly empty round of workgroup slots (2140 workgroups = 4.18 rounds of the 512 slots ->
   * 8.36 half-length rounds).  Needs 2 * nb0 * nb1 * heads * lq * SEVA_ATTN_SPLIT_ROW_FLOATS floats (per half and query row: 64 of
   * the un-normalised output, the running maximum and the row sum); NULL = never split. */
  float* split_ws;
  int64_t split_ws_bytes;
} seva_attn_desc;
int seva_attention_f16(const seva_attn_desc* d, seva_stream_t stream);

/* fp8 P.V attention (ABI 9; the opt-in `attention="fp8"` sub-option of the fp8 precision mode): the same operator for the long
 * sequences (lq >= SEVA_ATTN_LONG_MIN_LQ) with P and V in OCP e4m3 on the block-scaled MFMA; Q K^T stays f16.  V is first quantised into a private
 * workspace -- e4m3 values in the kernel's key order plus one E8M0 (power-of-two) scale byte per 32 keys and channel, per sample,
 * keys >= lk zero-padded -- by seva_attn_quant_v_fp8, which reads d->v through the k strides (nb0 / nb1 / token); then
 * seva_attention_pv8 reads q, k (f16, the desc's strides), the quantised V and writes out.  q must be pre-scaled (q_prescaled);
 * split_ws as for seva_attention_f16 (the split is a function of lk alone).  The row sum is taken from the quantised P, the
 * probabilities stay below 2^8 (rescale whenever a score passes the running reference by 8).  Accuracy class of the fp8 mode.
 * seva_attn_v_fp8_size: bytes of the two workspace parts for `batch` = nb0 * nb1 samples. */
int seva_attn_v_fp8_size(int32_t batch, int32_t heads, int32_t lk, int64_t* v8_bytes, int64_t* scale_bytes);
int seva_attn_quant_v_fp8(const seva_attn_desc* d, void* v8, uint8_t* v8_scale, seva_stream_t stream);
int seva_attention_pv8(const seva_attn_desc* d, const void* v8, const uint8_t* v8_scale, seva_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GroupNorm (fp32 statistics) over a channels-last tensor that may be the channel
 * concatenation of two sources (the UNet skip concat, seva/model.py:206-207, is never
 * materialised), optionally followed by SiLU and the Pluecker scale/shift modulation
 *   y = silu(gn(x)) * (1 + scale) + shift,  [scale|shift] = dense_w @ dense[n][p][:] + dense_b
 * Replaces GroupNorm32 + SiLU + dense_emb_layers of seva/modules/layers.py:61-63,98-100,
 * 106-111,122-131, the output head norm (seva/model.py:171) and the transformer input norm
 * (seva/modules/transformer.py:186,231).
 * workspace: at least n * SEVA_GN_WORKSPACE_SLABS * groups * 2 floats (that many slab slots per sample).
 */
#define SEVA_GN_WORKSPACE_SLABS 1024
typedef struct seva_groupnorm_desc {
  const float* x1; /* [n][hw][c1] */
  const float* x2; /* [n][hw][c2] or NULL */
  const float* gamma;
  const float* beta;    /* [c1 + c2] */
  const float* dense;   /* [n][hw][dense_c] or NULL */
  const float* dense_w; /* [2*(c1+c2)][dense_c] */
  const float* dense_b; /* [2*(c1+c2)] */
  void* out_f16;        /* [n][hw][c1+c2] */
  float* workspace;
  int32_t n, hw, c1, c2, groups, dense_c, silu;
  float eps;
  /* optional second output: the un-normalised (concatenated) input cast to f16, [n][hw][c1+c2] -- the A operand of
   * the ResBlock's 1x1 skip convolution (seva/modules/layers.py:137), written in the same pass instead of by a
   * separate seva_cast_concat_f16 read of both sources.  NULL = off. */
  void* raw_f16;
  /* optional e4m3 output (saturating, NaN kept), same layout: the A operand of seva_gemm_fp8 / an fp8 conv.  When set, out_f16
   * may be NULL. */
  void* out_f8;
  int64_t ld_out_f8; /* pixel pitch of out_f8 in bytes (>= c1 + c2; 0 = c1 + c2): lets a 320-channel tensor feed an fp8 conv whose
                      * channel count is padded to a multiple of 128 (pad bytes are never written: keep them zero) */
  /* optional: per-channel partial statistics of x1 / x2 as written by the kernel that produced them
   * (seva_gemm_desc.ch_stats: [n * hw / SEVA_CH_STATS_ROWS][2][c]).  When given for every source, the statistics pass over the fp32
   * tensors is skipped (x1 / x2 are then read once, by the apply pass).  Requires hw % SEVA_CH_STATS_ROWS == 0 (a block then
   * belongs to one sample and a sample's statistics stay bitwise independent of the batch). */
  const float* stats1;
  const float* stats2;
  /* split-precision outputs (ABI 7).  Non-zero: the output has pixel pitch 2 * (c1 + c2); channels [0, C) hold hi = f16(v) as
   * usual and channels [C, 2C) lo = f16(v - f32(hi)).  A consumer GEMM / conv whose weights are duplicated over the two
   * halves then sees the operand to ~22 bits (fp32 accumulation of hi * w + lo * w).  Used for the three operand roundings
   * that dominate the network's error (tests/test_f16_floor_cpu.py): the head conv's input (split_out_f16) and the 1x1 skip
   * convs' input (split_raw_f16).  Plain (non-modulated) and 6-component-modulated GroupNorms only. */
  int32_t split_out_f16;
  int32_t split_raw_f16;
} seva_groupnorm_desc;
int seva_groupnorm_f16(const seva_groupnorm_desc* d, seva_stream_t stream);

/* LayerNorm over the last dim, fp32 in, f16 out (nn.LayerNorm, transformer.py:102-104,124,141-143). */
int seva_layernorm_f16(const float* x, const float* gamma, const float* beta, void* out_f16,
                       int64_t rows, int32_t c, float eps, seva_stream_t stream);
/* Same normalisation as a split-precision operand (no ABI change: a new symbol only): out_f16 is [rows][2 c]; columns [0, c) hold
 * hi = f16(y), bit for bit seva_layernorm_f16's output, columns [c, 2 c) hold lo = f16(y - f32(hi)).  Against weights duplicated
 * [W | W] (K = 2 c) the fp32-accumulating MFMA then sees the normalised row to ~22 bits. */
int seva_layernorm_f16_split(const float* x, const float* gamma, const float* beta, void* out_f16,
                             int64_t rows, int32_t c, float eps, seva_stream_t stream);
/* Same normalisation with OCP e4m3 output (saturating at +-448; NaN stays NaN, byte 0x7F / 0xFF): the A operand of seva_gemm_fp8. */
int seva_layernorm_fp8(const float* x, const float* gamma, const float* beta, void* out_f8, int64_t rows,
                       int32_t c, float eps, int64_t ld_out /* row pitch in bytes, >= c; 0 = c; pad bytes untouched */,
                       seva_stream_t stream);

/* Row softmax: out[r][c] = softmax_c(x[r][c] * scale) as f16 for c < cols; columns cols..cols_pad-1
 * of `out` are written as 0 (so `out` can be the K-padded A operand of the following P*V GEMM).
 * Used for the single-head, d=512 attention of the VAE mid block, which runs as
 * GEMM(QK^T) -> softmax -> GEMM(PV) (diffusers AutoencoderKL decoder, reference autoencoder.py:38). */
int seva_softmax_rows_f16(const float* x, int64_t ldx, void* out_f16, int64_t ldo, int64_t rows,
                          int32_t cols, int32_t cols_pad, float scale, seva_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Layout / elementwise helpers.
 */
/* [n][c][h][w] f32 (two sources concatenated on c; second may be NULL) -> [n][h*w][cpad] f16,
 * channels >= c1+c2 zero-filled.  Replaces torch.cat at seva/model.py:227 + the NCHW->NLC
 * rearranges (transformer.py:232). `scale` (per-n, may be NULL) multiplies source 1 (c_in of
 * the denoiser, sampling.py:149). */
int seva_nchw_to_nhwc_f16(const float* x1, int32_t c1, const float* x2, int32_t c2,
                          const float* scale, void* out_f16, int32_t n, int32_t hw, int32_t cpad,
                          seva_stream_t stream);
/* Same, split precision (ABI 7): channels [C, 2C), C = c1 + c2, receive lo = f16(v - f32(f16(v))) of the value whose f16(v)
 * sits in [0, C); cpad >= 2C.  The stem conv (model.py:103) has 11 real channels in one 64-channel K-tile, so with its weights
 * duplicated over [C, 2C) the network input enters at ~22 bits for free. */
int seva_nchw_to_nhwc_f16_split(const float* x1, int32_t c1, const float* x2, int32_t c2,
                                const float* scale, void* out_f16, int32_t n, int32_t hw, int32_t cpad,
                                seva_stream_t stream);
/* [rows][ld] f32 channels-last -> [n][c][hw] f32 (first c channels). */
int seva_nhwc_to_nchw_f32(const float* x, int64_t ld, float* out, int32_t n, int32_t c,
                          int32_t hw, seva_stream_t stream);
/* concat-cast: [rows][c1] f32 ‖ [rows][c2] f32 -> [rows][c1+c2] f16 (x2 may be NULL). */
int seva_cast_concat_f16(const float* x1, int32_t c1, const float* x2, int32_t c2, void* out_f16,
                         int64_t rows, seva_stream_t stream);
/* Same, split precision (the contract of seva_nchw_to_nhwc_f16_split for the channels-last cast): out_f16 is [rows][2 C],
 * C = c1 + c2; columns [0, C) hold f16(v), columns [C, 2C) hold lo = f16(v - f32(f16(v))). */
int seva_cast_concat_f16_split(const float* x1, int32_t c1, const float* x2, int32_t c2, void* out_f16,
                               int64_t rows, seva_stream_t stream);
/* Bilinear resize, align_corners=True, [n][c][sh][sw] f32 -> channels-last [n][oh*ow][c] f32
 * (F.interpolate at seva/modules/layers.py:126-130; step-invariant). */
int seva_bilinear_to_nhwc_f32(const float* src, float* out, int32_t n, int32_t c, int32_t sh,
                              int32_t sw, int32_t oh, int32_t ow, seva_stream_t stream);
/* Sinusoidal timestep embedding cos(t*f)||sin(t*f) (layers.py:11-32), f16 out [n][dim]; t is
 * int64; freqs = exp(-ln(max_period) * arange(dim/2) / (dim/2)) as an f32 device table. */
int seva_timestep_embedding_f16(const int64_t* t, const float* freqs, void* out_f16, int32_t n,
                                int32_t dim, seva_stream_t stream);
/* out = silu(x) as f16 (nn.SiLU before emb_layers / inside time_embed). */
int seva_silu_f16(const float* x, void* out_f16, int64_t count, seva_stream_t stream);
/* out[i] = a[i] + b[i] (SkipConnect, transformer.py:158-165), fp32. */
int seva_add_f32(const float* a, const float* b, float* out, int64_t count, seva_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sampler elementwise (seva/sampling.py).  x tensors are [n][c][h][w] f32, `chw` = c*h*w.
 */
/* DiscreteDenoiser input blend, sampling.py:146-148:  out = x*(1-mask) + lat*mask, where
 * replace = [n][c+1][hw] holds (lat, mask). */
int seva_replace_blend_f32(const float* x, const float* replace, float* out, int32_t n, int32_t c,
                           int32_t hw, seva_stream_t stream);
/* out = net * c_out[n] + x * c_skip[n]  (sampling.py:149-152). */
int seva_denoiser_combine_f32(const float* net, const float* x, const float* c_out,
                              const float* c_skip, float* out, int32_t n, int64_t chw,
                              seva_stream_t stream);
/* x += eps * noise_scale[n]  (sampler_step, sampling.py:359-362); in-place allowed. */
int seva_add_noise_f32(const float* x, const float* eps, const float* noise_scale, float* out,
                       int32_t n, int64_t chw, seva_stream_t stream);
/* CFG + Euler update in one pass (sampling.py:204-213,364-368):
 *   den = u + scale[n]*(c - u);  d = (x - den)/sigma_hat[n];  out = x + dt[n]*d
 * `den2` = [2n][chw] with the uncond half first. */
int seva_cfg_euler_f32(const float* x, const float* den2, const float* scale,
                       const float* sigma_hat, const float* dt, float* out, int32_t n, int64_t chw,
                       seva_stream_t stream);
/* CFG + DPM-Solver++(2M) update in one pass (the `dpmpp2m` solver of seva/sampling.py; sgm's DPMPP2MSampler with
 * mult1 = a, -mult2*mult3 = b, mult2*mult4 = c):
 *   D = scale ? u + scale[n]*(cd - u) : den;   out = a[n]*x + b[n]*D + c[n]*old_den;   den_out = D
 * scale != NULL: `den` = [2n][chw] with the uncond half first; scale == NULL: `den` = [n][chw], already combined.
 * Where c[n] == 0 the history term is not evaluated at all (a select, not a multiply): a NaN/Inf in `old_den` cannot
 * reach `out`.  old_den == NULL means "no history term"; the caller guarantees c[n] == 0 for every n then (the entry
 * cannot check device values without a sync).  den_out may be NULL (D is not kept), may alias old_den; out may alias x. */
int seva_cfg_multistep_f32(const float* x, const float* den, const float* scale, const float* old_den,
                           const float* a, const float* b, const float* c, float* out, float* den_out,
                           int32_t n, int64_t chw, seva_stream_t stream);

/* Classifier-free guidance combine alone (ConstantGuidance, sampling.py:204-213):
 *   out = u + scale[n]*(c - u), den2 = [2n][chw] with the uncond half first. */
int seva_cfg_combine_f32(const float* den2, const float* scale, float* out, int32_t n, int64_t chw,
                         seva_stream_t stream);
/* Rescaled guidance (Lin et al. 2024, `guidance_rescale` of diffusers; `EulerEDMSampler(guidance_rescale=phi)`): the guided
 * prediction of each frame scaled towards the standard deviation of that frame's conditional prediction.
 * `den2` = [2n][chw] with the uncond half first and `scale` = [n], as seva_cfg_combine_f32 takes them.  Per frame f, N = chw:
 *   g_i  = u_i + scale[f]*(c_i - u_i)          the very device function of seva_cfg_combine_f32: phi == 0 gives its bits
 *   S1c = sum c_i, S2c = sum c_i^2, S1g = sum g_i, S2g = sum g_i^2      in fp64, no atomics: thread t of the frame's one
 *          256-thread workgroup adds elements t, t + 256, ... in that order, then the fixed tree of csrc/frame_common.h.
 *          The order depends on chw alone -- not on n, on the frame's position in the batch, or on anything else in the launch
 *   var_c = S2c - S1c^2/N,  var_g = S2g - S1g^2/N                        fp64 (a ratio of the two: no N vs N - 1 convention)
 *   m    = phi > 0 && var_g > 0 && var_c >= 0 ? phi*sqrt(var_c/var_g) + (1 - phi) : 1      a select: N = 1, phi == 0, and a
 *          constant frame whose sums are exact in fp64 (var == 0) give exactly 1; so does a NaN variance
 *   m32  = (float)m, rounded once;  out_i = m32 * g_i, one fp32 multiply;  mult_out[f] = m32 where mult_out != NULL
 * Non-finite inputs propagate through g.  `out` may not alias `den2`.  phi outside [0, 1] (NaN included), a NULL or
 * misaligned pointer, n <= 0 or chw <= 0: SEVA_ERR_ARG. */
int seva_cfg_rescale_f32(const float* den2, const float* scale, float phi, float* out, float* mult_out, int32_t n,
                         int64_t chw, seva_stream_t stream);
/* Euler step alone (to_d + update, sampling.py:24-25,366-368): out = x + dt[n]*(x - den)/sigma[n]. */
int seva_euler_step_f32(const float* x, const float* den, const float* sigma_hat, const float* dt,
                        float* out, int32_t n, int64_t chw, seva_stream_t stream);
/* d = (x - den)/sigma[n]  (to_d, sampling.py:24-25). */
int seva_to_d_f32(const float* x, const float* den, const float* sigma, float* out, int32_t n,
                  int64_t chw, seva_stream_t stream);
/* out = x * s[n] (input * c_in, sampling.py:150); in-place allowed. */
int seva_scale_rows_f32(const float* x, const float* s, float* out, int32_t n, int64_t chw,
                        seva_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Conditioning geometry.
 * Pluecker ray maps, seva/geometry.py:119-165 (get_plucker_coordinates) with get_center_and_ray
 * (102-116) and get_image_grid (82-89): out[v][0:3][y][x] = unit ray direction of latent pixel
 * (x+0.5, y+0.5) of view v, out[v][3:6] = camera centre x direction, all in the source camera's frame.
 * kinv [views][9]: row-major inverse of view v's intrinsics in latent-pixel units;
 * pose_inv [views][12]: rows of inverse(to_hom(extrinsics_rel[v]))[:3, :4] (the two small matrix inverses
 * per view stay on the host, as in the reference).  out: [views][6][h][w] fp32.
 */
int seva_plucker_f32(const float* kinv, const float* pose_inv, float* out, int32_t views, int32_t h,
                     int32_t w, seva_stream_t stream);
/* Channel assembly of do_sample (seva/eval.py:1255-1270): c_concat[v] = [mask[v] broadcast | plucker[v]],
 * uc_concat[v] = [0 | plucker[v]]; both [views][7][h][w] fp32; mask: one byte per view. */
int seva_cond_concat_f32(const float* plucker, const uint8_t* mask, float* c_concat, float* uc_concat,
                         int32_t views, int32_t h, int32_t w, seva_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CLIP ViT-H-14 image conditioner (seva/modules/conditioner.py:7-39).  Its GEMMs / LayerNorms are
 * seva_gemm_f16 / seva_layernorm_*; these three entry points are what those cannot express.
 */
/* LayerNorm with fp32 output (CLIP's ln_pre: the result IS the residual stream).  No overlap of x and out. */
int seva_layernorm_f32(const float* x, const float* gamma, const float* beta, float* out_f32, int64_t rows,
                       int32_t c, float eps, seva_stream_t stream);
/* conditioner.py:24-34: kornia.geometry.resize(x, (out,out), bicubic, align_corners=True, antialias) -> (x+1)/2 ->
 * normalize(mean, std); x: [n][3][H][W] fp32 in [-1,1].  The result is written as the f16 patch matrix of the
 * patch x patch / stride-patch embedding conv: row = image * (out/patch)^2 + py * (out/patch) + px, column =
 * (c * patch + ky) * patch + kx (= conv weight .reshape(width, 3*patch*patch)); columns beyond 3*patch^2 are untouched. */
int seva_clip_preprocess_f16(const float* x, void* patches_f16, int32_t n, int32_t H, int32_t W, int32_t out_size,
                             int32_t patch, int32_t ld_patches, const float* mean, const float* std,
                             int32_t antialias, seva_stream_t stream);
/* softmax(q k^T * scale) v for short sequences and any even head dim <= 128 (ViT-H-14: L = 257, d = 80), f16 in/out,
 * fp32 math.  Element (b, token l, head h, d) of q at q + b*q_sb + l*q_sl + h*head_dim + d; k, v share strides. */
int seva_attention_small_f16(const void* q, const void* k, const void* v, void* out, int64_t q_sb, int64_t q_sl,
                             int64_t k_sb, int64_t k_sl, int64_t o_sb, int64_t o_sl, int32_t batch, int32_t heads,
                             int32_t L, int32_t head_dim, float scale, seva_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Image front and back end (seva/eval.py:160-322 load_img_and_K / transform_img_and_K, 974-975 save_output).
 *
 * One kernel fuses source conversion, alpha compositing, F.interpolate(mode="area"), crop or pad and an affine output
 * map; only the H x W output pixels are computed (the reference resizes the whole image, then crops).  The arithmetic
 * is the reference's CPU expression operation by operation, every fp32 operation rounded on its own (no FMA, correctly
 * rounded divisions), so the result equals the reference's bit for bit:
 *   uint8 source     v = float(u8) / 255.0f
 *   4 channels       v = rgb * a + bg * (1 - a): mul, sub, mul, add; bg = 1.0f, or context_rgb when given
 *   area             resized pixel (i, j) = mean of source rows floor(i*h/rh) .. ceil((i+1)*h/rh) - 1 and columns
 *                    floor(j*w/rw) .. ceil((j+1)*w/rw) - 1: summed in fp32 in row-major order starting from 0, then
 *                    divided by the row count, then by the column count (a 1 x 1 window copies the value)
 *   window           out[y][x] = resized[ct + y][cl + x]; (ct, cl) is signed and a pixel outside the resized image
 *                    takes pad_value
 *   output           v * out_mul + out_add as two operations, padding pixels included, skipped when (out_mul,
 *                    out_add) == (1, 0)
 * The result of an image depends on nothing but that image: not on n, on the pitches or on what surrounds the output;
 * only the H x W pixels of each of the 3 planes of an image are written.
 */
typedef struct seva_image_desc {
  const void* src;          /* u8: [n][h][w][src_c], src_c = 3 (RGB) or 4 (RGBA); f32: [n][3][h][w] */
  const float* context_rgb; /* optional alpha background, fp32 [h][w][3] dense, shared by the n images (src_c = 4 only);
                               NULL = white */
  float* out;               /* [n][3][H][W] fp32: planes and rows dense, images out_pitch_n floats apart */
  int64_t src_pitch_n;      /* source elements (u8: bytes, f32: floats) between images, */
  int64_t src_pitch_c;      /*   between channel planes (f32 only), */
  int64_t src_pitch_row;    /*   between rows; src_c = 4 reads a pixel as one 32-bit word: src and both pitches % 4 == 0 */
  int64_t out_pitch_n;      /* >= 3*H*W */
  int32_t n, h, w, src_c;
  int32_t rh, rw;           /* size of the resized image, never materialised */
  int32_t ct, cl;           /* origin of the output window inside it (signed) */
  int32_t H, W;
  float pad_value, out_mul, out_add;
} seva_image_desc;
int seva_image_area_crop_u8(const seva_image_desc* d, seva_stream_t stream);
int seva_image_area_crop_f32(const seva_image_desc* d, seva_stream_t stream);
/* save_output's frame rule (eval.py:974-975): x [n][3][H][W] fp32, images x_pitch_n floats apart -> out [n][H][W][3] uint8
 * dense; t = (v + 1.0f) / 2.0f; t = t * 255.0f; clamp to [0, 255]; truncate -- separate fp32 operations.  +-inf clamp to
 * 255 / 0.  NaN writes 0: the reference leaves NaN -> uint8 undefined (the result of a C++ cast), this is this
 * library's choice. */
int seva_rgb_to_u8(const float* x, int64_t x_pitch_n, uint8_t* out, int32_t n, int32_t H, int32_t W,
                   seva_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Image-space scores: per-frame squared error (-> MSE / PSNR) and SSIM of two batches of frames, on the uint8 values a
 * user would save.  New symbols and one new struct; no existing struct changes (ABI version unchanged).
 *
 *   inputs     a, b: n frames H x W x 3 each, both of one kind.  kind 0: uint8 [n][H][W][3], rows and pixels dense,
 *              images *_pitch_n BYTES apart.  kind 1: fp32 [n][3][H][W] in [-1, 1], planes and rows dense, images
 *              *_pitch_n FLOATS apart; every value goes through the rule of seva_rgb_to_u8 as it is loaded
 *              ((v + 1) / 2 * 255, clamp, truncate, NaN -> 0), so both kinds score the same integers.
 *   sse        sse[i] = sum over the H*W*3 elements of (a - b)^2, exact, int64.
 *   ssim       Wang et al. 2004, per channel: 11-tap Gaussian window, sigma 1.5, g[k] = exp(-(k-5)^2 / 4.5) normalised
 *              to sum 1 in fp64 and rounded once to fp32, applied separably (along a row first, then down the column)
 *              at "valid" positions only: (H-10) x (W-10) per channel.  All arithmetic is fp32, every operation rounded
 *              on its own (no FMA), on x = float(a), y = float(b):
 *                each pass:  acc = 0; for k = 0..10: acc = acc + g[k] * v[k]        (v = x, y, x*x, y*y, x*y in the row
 *                            pass; the row pass's five results in the column pass)
 *                moments:    mx, my, exx, eyy, exy;  mxx = mx*mx, myy = my*my, mxy = mx*my;
 *                            sx = exx - mxx, sy = eyy - myy, sxy = exy - mxy                         (biased)
 *                map:        ((2*mxy + C1) * (2*sxy + C2)) / (((mxx + myy) + C1) * ((sx + sy) + C2)), one correctly
 *                            rounded division;  C1 = (0.01*255)^2 = 6.5025f, C2 = (0.03*255)^2 = 58.5225f
 *              The two frames' expressions are the same operations in the same order: a frame against itself gives
 *              exactly 1.0 at every position.  Each position's fp32 value is widened to fp64 and summed:
 *              ssim_sum[i] = sum over 3 channels and all valid positions; the caller divides by 3 (H-10) (W-10).
 *              ssim_map (optional): the fp32 values, [n][3][H-10][W-10] dense.
 *   reduction  one workgroup per 32 x 32 tile of an image; the threads' partials are summed by a fixed binary tree, one
 *              (fp64 SSIM sum, u32 squared error) pair per tile goes into the workspace, and a second kernel sums an
 *              image's tiles in a fixed order.  No atomics: results repeat bit for bit and depend on nothing but the
 *              image itself -- not on n, on the pitches, on what else runs or on what surrounds the outputs.
 * ssim != 0 needs ssim_sum and H, W >= 11 (error otherwise); ssim == 0 computes sse only, for any H, W >= 1, and
 * ssim_sum / ssim_map must then be NULL.  seva_frame_metrics_size: bytes of `workspace` (8-byte aligned). */
typedef struct seva_metrics_desc {
  const void* a;            /* generated frames */
  const void* b;            /* target frames, same kind and shape */
  int64_t* sse;             /* [n] */
  double* ssim_sum;         /* [n]; NULL when ssim == 0 */
  float* ssim_map;          /* optional [n][3][H-10][W-10] */
  void* workspace;          /* seva_frame_metrics_size bytes; contents need not be kept between calls */
  int64_t a_pitch_n;        /* kind 0: bytes, kind 1: floats; >= 3*H*W */
  int64_t b_pitch_n;
  int64_t workspace_bytes;
  int32_t n, H, W;
  int32_t kind;             /* 0: uint8 NHWC, 1: fp32 NCHW */
  int32_t ssim;             /* 0: sse only */
} seva_metrics_desc;
int seva_frame_metrics_size(int32_t n, int32_t H, int32_t W, int64_t* workspace_bytes);
int seva_frame_metrics(const seva_metrics_desc* d, seva_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * LPIPS v0.1 with the VGG-16 backbone (Zhang et al. 2018; spatial = False, normalize = False): the three operators around the 13
 * convolutions, which are seva_gemm_f16 in conv mode writing out_f16.  New symbols and one new struct; no existing struct
 * changes (ABI version unchanged).  All fp32 arithmetic below is rounded operation by operation (no FMA; divisions and square
 * roots correctly rounded), in the stated order.
 *
 * Input preparation: the scaling layer's output as the first conv's operand.
 *   src        n frames H x W x 3.  kind 0: uint8 [n][H][W][3], rows and pixels dense, images src_pitch_n BYTES apart; the
 *              byte is u.  kind 1: fp32 [n][3][H][W] in [-1, 1], planes and rows dense, images src_pitch_n FLOATS apart;
 *              u is the value after the rule of seva_rgb_to_u8 ((v + 1) / 2 * 255, clamp, truncate, NaN -> 0): both kinds
 *              feed the tower the same integers, those seva_frame_metrics scores.
 *   out_f16    [n][H][W][64] f16 dense.  Channel c < 3:  x = float(u) / 127.5f;  x = x - 1.0f;  x = x - shift[c];
 *              x = x / scale[c];  one round-to-nearest-even to f16;  shift = (-.030f, -.088f, -.188f), scale = (.458f, .448f,
 *              .450f).  Channels 3..63 are written as exactly zero (the padded K of the first conv). */
int seva_lpips_prepare_f16(const void* src, int64_t src_pitch_n, int32_t kind, void* out_f16, int32_t n, int32_t H,
                           int32_t W, seva_stream_t stream);
/* ReLU, with the 2 x 2 / stride-2 max-pool where asked.  x: [n][h][w][c] f16 dense, c % 64 == 0 (a conv's out_f16).
 *   relu_out   [n][h][w][c]: x > 0 ? x : 0, a NaN stays a NaN (torch.relu).  May be x itself (in place).
 *   pool_out   NULL, or [n][h/2][w/2][c]: the maximum of relu_out over rows 2i, 2i+1 and columns 2j, 2j+1, a NaN in the
 *              window gives a NaN (torch max_pool2d); floor semantics, an odd last row or column is dropped.  h, w >= 2.
 * Nothing but the n*h*w*c (+ n*(h/2)*(w/2)*c) elements is written. */
int seva_lpips_relu_pool_f16(const void* x, void* relu_out, void* pool_out, int32_t n, int32_t h, int32_t w, int32_t c,
                             seva_stream_t stream);
/* Layer distance: out[i] = sum over the hw pixels of pair i of d, the caller divides by hw.
 *   fa, fb     features of the two frames of a pair, f16 [n][hw][C], pixels and channels dense, pairs *_pitch_n ELEMENTS
 *              apart; C = 64, 128, 256 or 512.   w: fp32 [C], the layer's linear weights (>= 0).
 *   per pixel  L = C / 8 lanes; lane j holds channels 8j .. 8j+7 of both vectors, widened to fp32 (a_i, b_i).
 *                squares:   s = 0; for i = 0..7: s = s + a_i * a_i                                       (likewise for b)
 *                butterfly: for o = L/2, L/4, .. 1: s = s + s[lane ^ o]        (every lane ends with the same value)
 *                norm:      ra = 1.0f / (sqrt(s) + 1e-10f)        (one division per vector, not one per channel; likewise rb)
 *                distance:  d = 0; for i = 0..7: df = a_i * ra - b_i * rb;  d = d + w_i * (df * df);  then the butterfly
 *              The two vectors' expressions are the same operations in the same order and (x - y)^2 == (y - x)^2 exactly:
 *              a frame against itself gives exactly 0.0, and swapping fa and fb changes no bit.
 *   reduction  a pixel's fp32 d is widened to fp64.  One 256-thread workgroup per 256 consecutive pixels of a pair: with
 *              G = 256 / L, thread g*L of the workgroup adds the d of pixels g, g + G, g + 2G, .. of the chunk in that order
 *              (every other thread holds 0), the 256 values go through the binary tree v[t] += v[t + s], s = 128 .. 1, into
 *              workspace[pair][chunk]; a second kernel, one workgroup per pair, has thread t add chunks t, t + 256, .. in
 *              that order and applies the same tree.  No atomics: results repeat bit for bit and depend on nothing but
 *              the pair itself -- not on n, on the pitches or on what surrounds out and the workspace.
 * seva_lpips_layer_size: bytes of `workspace` (8-byte aligned; contents need not be kept between calls). */
typedef struct seva_lpips_layer_desc {
  const void* fa;           /* f16 [n][hw][C] */
  const void* fb;
  const float* w;           /* [C] */
  double* out;              /* [n] */
  void* workspace;
  int64_t a_pitch_n;        /* f16 elements between pairs, >= hw*C, % 8 == 0 */
  int64_t b_pitch_n;
  int64_t workspace_bytes;
  int64_t hw;
  int32_t n, C;
} seva_lpips_layer_desc;
int seva_lpips_layer_size(int32_t n, int64_t hw, int64_t* workspace_bytes);
int seva_lpips_layer(const seva_lpips_layer_desc* d, seva_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Dynamic-range audit of one tensor: exponent histogram, special-value counts and finite extrema in one pass.  New symbols and
 * one new struct; no existing struct changes (ABI version unchanged).  Everything is decided by integer tests on the elements' bit
 * patterns (every f16 and e4m3 value is exact in f32), so denormal-flush modes do not enter; all counts are exact integers.
 *   x          rows x cols elements, unit inner stride, rows `pitch` ELEMENTS apart (>= cols), aligned to the element size.
 *              dtype SEVA_RANGE_F32, SEVA_RANGE_F16, or SEVA_RANGE_E4M3 (bytes in the OCP e4m3 "fn" encoding: no infinity,
 *              NaN = 0x7F / 0xFF -- the encoding of every e4m3 tensor of this library).  Only the rows x cols elements are read.
 *   out        SEVA_RANGE_WORDS uint64 words, device memory, 8-byte aligned.  With e(x) = floor(log2 |x|) of the exact value
 *              (subnormals of the format included):
 *                [0]            elements equal to +-0
 *                [1 + k]        k = 0..63: finite non-zero elements with clamp(e(x), -32, 31) == k - 32
 *                [65]           +-inf (always 0 for e4m3)
 *                [66]           NaN, any payload
 *                [67]           elements with |x| equal to the format's largest finite value (65504, 448, FLT_MAX); they are
 *                               counted in their exponent bin as well -- the saturation signal of the e4m3 producers
 *                [68]           f32 bit pattern of the largest finite |x|; 0 if there is none
 *                [69]           f32 bit pattern of the smallest finite non-zero |x|; 0x7F800000 if there is none
 *                [70]           rows * cols == [0] + sum [1..64] + [65] + [66]
 *                [71]           0
 *   workspace  seva_tensor_range_size(rows, cols) bytes, 8-byte aligned; contents need not be kept between calls.  It holds one
 *              partial table per workgroup of the counting kernel; workgroup w counts elements [w * S, (w + 1) * S) of the
 *              row-major rows x cols index space, S = SEVA_RANGE_WG_ELEMS (a larger multiple of it above SEVA_RANGE_MAX_WGS * S elements), and
 *              a second kernel adds the tables.  No atomics in global memory; the result is independent of the split.
 * Nothing but the SEVA_RANGE_WORDS words and the workspace is written.  rows * cols <= 2^46. */
enum { SEVA_RANGE_F32 = 0, SEVA_RANGE_F16 = 1, SEVA_RANGE_E4M3 = 2 };
#define SEVA_RANGE_WORDS 72
#define SEVA_RANGE_WG_ELEMS 32768
#define SEVA_RANGE_MAX_WGS 2048 /* most workgroups (partial tables of the workspace) of the counting kernel */
typedef struct seva_range_desc {
  const void* x;
  int32_t dtype;
  int64_t rows, cols, pitch;   /* pitch in elements, >= cols */
  void* workspace;
  int64_t workspace_bytes;
  uint64_t* out;               /* SEVA_RANGE_WORDS words, device memory */
} seva_range_desc;
int seva_tensor_range_size(int64_t rows, int64_t cols, int64_t* workspace_bytes);
int seva_tensor_range(const seva_range_desc* d, seva_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Benchmark / debugging knobs. The library reads its SEVA_* environment variables ONCE, when it is loaded (nothing
 * on the launch path calls getenv); a host changes a knob at run time with seva_set_knob (tests, tools).  Names:
 * gemm_chunks, gemm_dbg, gemm_stagger, gemm_bm, gemm_bn, gemm_astat, attn_dbg, attn_no_tr, attn_two, attn_split,
 * attn_short2 (32 < lq <= 64 and lk <= 64: 1 = two waves on one K/V buffer, 0 = the four-wave kernel; same bits), gn_min_iter, conv_win (0: per-tap conv gather everywhere; 1 / 2: force the 4-wave / 8-wave family of the window-staged conv kernel)
 * (environment: SEVA_ + upper case).  -1 = unset (default heuristics).  None is needed in production.
 */
int seva_set_knob(const char* name, int32_t value);
int seva_get_knob(const char* name, int32_t* value);

/* ------------------------------------------------------------------------------------------
 * hipGraph helpers: capture everything enqueued on `stream` between begin/end, replay later.
 */
int seva_graph_begin(seva_stream_t stream);
int seva_graph_end(seva_stream_t stream, void** graph_exec_out);
int seva_graph_launch(void* graph_exec, seva_stream_t stream);
int seva_graph_destroy(void* graph_exec);

/* ------------------------------------------------------------------------------------------
 * Per-kernel-class timing with HIP events on the launch stream (bench.py roofline leg).
 * Classes: 0 gemm, 1 conv, 2 attention, 3 norm, 4 elementwise.
 */
#define SEVA_PROF_CLASSES 5
int seva_prof_enable(int on);
/* Synchronises; fills ms[SEVA_PROF_CLASSES], launches[...], work[...] (algorithmic flop for classes 0-2, bytes for
 * 3-4) and bytes[...] (algorithmic HBM bytes: every operand read once, every result written once); resets. */
int seva_prof_collect(double* ms, int64_t* launches, double* work, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* SEVA_HIP_H */
