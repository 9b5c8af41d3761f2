// 3x3 / stride 1 / pad 1 convolution as implicit GEMM with the INPUT WINDOW of the output tile staged in LDS
// (reference: seva/modules/layers.py:101,113 -- the two 3x3 convs of every ResBlock; seva/model.py:57).
//
// gemm.hip's conv mode gathers one A tile per (tap, 64-channel slab): every input pixel of a tile crosses L2 -> LDS nine
// times (PMC, round 3: 4.1x the algorithmic bytes), and the LDS-DMA stream is what bounds that main loop.  Here the
// reduction runs slab-outer / tap-inner:
//
//   for each 64-channel slab s:   window = input pixels of the tile + halo, 128 B per pixel, staged ONCE
//     for each tap (ky, kx):      A fragments = window rows shifted by ky * (W + 2) + kx;  weight tile (tap, s) streamed
//
// The window is a contiguous range of a PADDED pixel index space: every image row gets ONE frame cell in front (the right
// frame of row r is the left frame of row r + 1), every image one frame row on top (the bottom frame of image i is the top
// frame of image i + 1), images stacked: with Wp = W + 1 and S = (H + 1) Wp, output pixel m = (img, y, x) sits at
// P(m) = img * S + (y + 1) Wp + (x + 1) and its tap (ky, kx) at P(m) + (ky - 1) Wp + (kx - 1), for every pixel of every image --
// border taps land on frame cells, which the fill routes to the zero page.  A tile of BM consecutive output pixels needs
// BM + (row crossings) + (W + 2 per image crossing) + 2 (W + 2) + 1 window pixels whatever its alignment, and the tap shift is
// one workgroup-uniform scalar.  Tiles are consecutive pixels of the whole launch where that fits the window capacity (36x36
// and smaller at 160 rows), consecutive pixels of ONE image otherwise (72x72); an output row gets the same bits either way.  Per slab and 160 x 160 tile the LDS-DMA traffic drops from
// 9 * (160 + 160) * 128 B = 360 KiB to 316 * 128 B + 9 * 160 * 128 B = 220 KiB; the weight tile is now the main stream.
//
// Everything else is the shared tile core (gemm_tile.h): K-tile 64, 128-byte LDS rows, lane-linear LDS-DMA with the natural chunk
// swizzle, weight fragment as the MFMA A operand, fp32 residual loaded straight into the accumulators, GroupNorm statistics from the
// epilogue.  The window's swizzle key is the WINDOW pixel index, so a tap shift that is not a multiple of 16 leaves some 2-way bank
// conflicts on the A fragment reads (measured: see DESIGN.md section 4).
//
// Wide images (the VAE decoder's 144 .. 576 px rows: a linear window of BM pixels + two image rows does not fit LDS): 2-D tiles of
// 16 output columns x BM / 16 output rows (TW = 16).  The window is the tile's (rows + 2) x 18 source pixels stored row after row
// (row pitch 18), MFMA block i of the tile is its row i, the tap shift is ky * 18 + kx -- the same uniform scalar -- and the halo costs
// 27 % more pixels than the tile has whatever the image width.  GroupNorm statistics blocks are then 4 tile rows x 16 pixels (any
// partition of an image's pixels into 64-pixel blocks serves the consumer, which sums the blocks of an image).
//
// NW = 4: two workgroups per CU (the window single-buffered: 320 px + two 160-row weight stages = 80 KiB each).
// NW = 8: one workgroup per CU on a 256-row tile, window double-buffered and refilled piece by piece under the taps.
#include "gemm_common.h"

#include <atomic>
#include <type_traits>

namespace {

constexpr int BK = 64;  // fp16 elements per K-tile -> 128-byte LDS rows

struct ConvWinGeom {
  uint32_t mul_hw, mul_iw, mul_sp, mul_wp;  // floor(2^32 / d) + 1: x / d == mulhi(x, mul) over the launch's range of x (host-checked)
  int32_t Wp, Sp, hw;                       // hw = OUTPUT pixels per image; mul_iw divides by the OUTPUT width ow
  int32_t ow;
  int32_t tiles_m, tiles_n;
  int32_t tpi;  // 0: M-tiles are consecutive BM-pixel ranges of the whole launch; > 0: tiles per image (a tile never leaves its image)
  int32_t n_lin;  // host only: images per launch of the linear tiles (31-bit offsets, exact multiply-high divisions); 0 = not even one
};  // filled from the plan (gemm_plan.h: WinGeom, WinTiling)

// UP: the conv input is the nearest-2x upsampled image (reference layers.py:35-46: F.interpolate(scale_factor=2) then conv): the window
// is staged from the SOURCE image and tap (ky, kx) of output pixel (y, x) reads source pixel ((y + ky - 1) >> 1, (x + kx - 1) >> 1)
// (A third weight stage with a counted vmcnt -- tap g + 2 issued under tap g, this tap's own DMA left in flight across the barrier -- was
// built and measured on the 8-wave family: 3 - 10 % SLOWER on every shape, profiles/r04_kconvwin_variants.log; removed.)
// FP8 (BASELINE config 5; gemm.hip's e4m3 scheme): a 128-byte window / weight row is 128 e4m3 channels instead of 64 f16 ones (cin, K and the
// pointers count 2-byte units, so every address here is unchanged); the two 16-byte fragment reads of a (tap, slab) form ONE 32-byte operand of
// v_mfma_scale_f32_16x16x128_f8f6f4, the per-output-channel power-of-two weight scale rides as the E8M0 block scale of the weight operand.
// The VAE decoder's fp8 mode adds e4m3 instantiations with 2-D tiles and with UP (both byte-agnostic above), and O8: the e4m3 output epilogue.
//
// S2 (the VAE encoder's fp8 mode: diffusers Downsample2D, 3x3 / stride 2 / padding on the bottom and right only): output pixel (y, x) reads
// source pixel (2y + ky, 2x + kx), never a negative one.  Stride-2 fragment rows would all sit on one parity of window pixels, i.e. on one
// 128-byte half of the 256-byte bank row: 2-way bank conflicts on every read whatever the chunk key.  So the window is stored COLUMN-PARITY
// SPLIT: even source columns first, odd ones behind them.  Fragment row i then reads slot base + i (consecutive slots, the stride-1 pattern and
// its chunk key), and tap (ky, kx) is still one uniform slot shift, ky * RP + (kx & 1) * HALF + (kx >> 1).
//   2-D tiles: a window of (2 TH + 1) source rows x 33 columns per 16 x TH output tile, each row stored as 17 even + 16 odd columns
//              (RP = 33, HALF = 17);
//   linear tiles: the padded index space with bottom / right frame cells only (P(m) = img * Sp + 2y Wp + 2x, Wp = iw + 1 rounded up to even so
//              that parity of P is parity of the column), split over the tile's window: even indices in slots [0, HALF), odd ones behind
//              (RP = Wp / 2, HALF = half the tile's window, a workgroup-uniform scalar).
//
// PH (seva_gemm_desc.upsample = 2; the three Upsample convs of a step): the nearest-2x upsample + 3x3 conv as FOUR 2x2 convs on the source
// image.  Output rows 2i and 2i + 1 read source rows {i-1, i, i} and {i, i, i+1}: the weight rows that meet on one source row are added on the
// host, columns alike, so output phase (py, px) is a 2x2 conv whose tap (a, b) sits at source offset (a + py - 1, b + px - 1) -- 4 taps and
// 4/9 of the FLOPs.  A workgroup computes ONE phase of a tile of consecutive SOURCE pixels: it is the plain kernel (same window, same
// fragment addresses) restricted to the taps (ky, kx) = (a + py, b + px), with the phase's own [N][4 cin] weight matrix and an epilogue
// that scatters source pixel (i, j) to output pixel (2i + py, 2j + px).  The four phases of a tile are neighbours in the remapped order
// (they stage the same window).  Plain fp32 epilogue with bias only; M, hw, ow of the arguments describe the SOURCE image.
// upsample = 4 is the same operator on the 128-column family (the VAE decoders' three upsample convs: 128 / 256 / 512 channels, 72 .. 288 px
// source rows): linear tiles where one image's windows fit, else 2-D tiles of 16 SOURCE columns x BM / 16 source rows -- the plain 2-D window
// of (rows + 2) x 18 source pixels, tap (a, b) of phase (py, px) the uniform shift (a + py) * 18 + (b + px) -- and GroupNorm statistics: a
// wave's 64 source pixels are 64 output pixels of one phase, written as block 4 * (source block) + phase (needs ih * iw % 64 == 0).
template <int BM, int BN, int NW, int WCAP, bool DBW, bool STATS, bool UP = false, int TW = 0, bool FP8 = false, bool O8 = false, bool S2 = false, bool PH = false>
__global__ __launch_bounds__(64 * NW, 2) void conv_win_kernel(GemmArgs p, ConvWinGeom g) {
  constexpr bool T2D = TW > 0;
  static_assert(TW == 0 || TW == 16, "2-D tiles are 16 output columns wide: an MFMA block is a tile row");
  static_assert(!O8 || FP8, "the e4m3 output epilogue belongs to the e4m3 instantiations");
  static_assert(!S2 || (FP8 && !UP && !O8), "stride 2: e4m3, no upsample, no e4m3 output (the encoder's downsample convs)");
  static_assert(!PH || (!UP && !FP8 && !S2), "phase mode: f16 operands on the source image");
  static_assert(!PH || (TW == 0 && !STATS) || BN == 128, "phase mode: 2-D tiles and statistics belong to the 128-column family");
  constexpr int NT = PH ? 4 : 9;                               // taps per slab
  constexpr int TH = BM / 16;                                  // output rows of a 2-D tile
  constexpr int SW2 = UP ? 8 : 16, SH2 = UP ? TH / 2 : TH;     // its source extent; window = (SH2 + 2) x (SW2 + 2) pixels
  constexpr int PITCH2 = S2 ? 33 : SW2 + 2, WL2 = S2 ? (2 * TH + 1) * 33 : (SH2 + 2) * PITCH2;
  static_assert(!T2D || (WL2 <= WCAP && TH % 2 == 0), "2-D window capacity");
  constexpr int WMW = NW / 2, WNW = 2;
  constexpr int WM = BM / WMW, WN = BN / WNW;  // per-wave tile
  constexpr int MI = WM / 16, NJ = WN / 16;
  static_assert(WM % 16 == 0 && WN % 16 == 0, "per-wave tile must be whole MFMA blocks");
  static_assert(!STATS || WM == 64, "statistics: a wave owns a 64-row block");
  constexpr int NPC = WCAP / 8, PPW = (NPC + NW - 1) / NW;  // window pieces (8 pixels x 128 B), per wave
  constexpr int NBP = BN / 8, BPW = (NBP + NW - 1) / NW;    // weight pieces per stage, per wave
  constexpr int WIN_BYTES = WCAP * 128, B_BYTES = BN * 128;
  constexpr int NWB = DBW ? 2 : 1;
  static_assert(WCAP % 8 == 0, "window capacity in whole pieces");
  static_assert(!DBW || PPW <= 8, "double-buffered window: one piece per wave and tap");

  extern __shared__ __attribute__((aligned(16))) char smem[];  // [window x NWB][weight stage 0][weight stage 1]
  const char* const lds_win = smem;
  const char* const lds_b = smem + NWB * WIN_BYTES;
  const unsigned lds_base_u32 = __builtin_amdgcn_readfirstlane(lds_addr_u32(smem));

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / WNW, wn = wave % WNW;
  const int sr = lane >> 3, sp = lane & 7;
  const int fr = lane & 15, fg = lane >> 4;

  const int work_ph = xcd_remap(blockIdx.x, g.tiles_m * g.tiles_n * (PH ? 4 : 1));
  const int ph = PH ? work_ph & 3 : 0, work = PH ? work_ph >> 2 : work_ph;  // PH: phase 2 py + px, the four of a tile side by side
  const int tm = work / g.tiles_n, tn = work - tm * g.tiles_n;  // sibling N-tiles of an M-tile are neighbours on one XCD
  // rows [m0, m_end) of the [M][N] output belong to this tile (2-D tiles: BM rows of ONE image that are not consecutive; see row_m)
  uint32_t m0, m_end;
  uint32_t t_img = 0, t_y0 = 0, t_x0 = 0, t_k = 0;  // 2-D: image, output origin of the tile, tile number inside the image
  if constexpr (T2D) {
    t_img = (uint32_t)tm / (uint32_t)g.tpi;
    t_k = (uint32_t)tm - t_img * (uint32_t)g.tpi;
    const uint32_t tpr = (uint32_t)g.ow / 16u, ty = t_k / tpr;
    t_y0 = ty * TH;
    t_x0 = (t_k - ty * tpr) * 16u;
    m0 = t_img * (uint32_t)g.hw;
    m_end = m0 + (uint32_t)g.hw;
  } else if (g.tpi > 0) {
    const uint32_t img = (uint32_t)tm / (uint32_t)g.tpi, k = (uint32_t)tm - img * (uint32_t)g.tpi;
    m0 = img * (uint32_t)g.hw + k * BM;
    m_end = m0 + BM < (img + 1) * (uint32_t)g.hw ? m0 + BM : (img + 1) * (uint32_t)g.hw;
  } else {
    m0 = (uint32_t)tm * BM;
    m_end = m0 + BM < (uint32_t)p.M ? m0 + BM : (uint32_t)p.M;
  }
  const int64_t n0 = (int64_t)tn * BN;
  // output row of MFMA block i (of this wave) and lane fr; linear tiles: may lie past the tile (m >= m_end: clamp for loads, no store)
  auto row_m = [&](int i) -> uint32_t {
    if constexpr (T2D) return m0 + (t_y0 + (uint32_t)(wm * (WM / 16) + i)) * (uint32_t)g.ow + t_x0 + (uint32_t)fr;
    else return m0 + (uint32_t)(wm * WM + 16 * i + fr);
  };
  const int pitch = T2D ? PITCH2 : g.Wp;  // window row pitch

  // padded index of the source pixel under the CENTRE tap of output pixel m (UP: of the pixel it is upsampled from); xo = its column
  auto pad_index = [&](uint32_t m, uint32_t& yo, uint32_t& xo) -> uint32_t {
    const uint32_t img = __umulhi(m, g.mul_hw);
    const uint32_t rem = m - img * (uint32_t)g.hw;
    yo = __umulhi(rem, g.mul_iw);
    xo = rem - yo * (uint32_t)g.ow;
    if constexpr (S2) return img * (uint32_t)g.Sp + 2u * yo * (uint32_t)g.Wp + 2u * xo;  // (S2: the source pixel under tap (0, 0))
    const uint32_t y = UP ? yo >> 1 : yo, x = UP ? xo >> 1 : xo;
    return img * (uint32_t)g.Sp + (y + 1) * (uint32_t)g.Wp + x + 1;
  };
  uint32_t q0 = 0;
  int WL = WL2, WS = WL2;  // window pixels; window slots (S2 linear: two halves of HALF slots)
  int s2_half = 17;        // S2: slot of the first odd column (2-D) / odd padded index (linear)
  if constexpr (!T2D) {
    uint32_t y_a, x_a, y_b, x_b;
    const uint32_t P0 = pad_index(m0, y_a, x_a), P1 = pad_index(m_end - 1, y_b, x_b);
    if constexpr (S2) {  // taps (ky, kx) of the tile's first .. last output pixel: [P0, P1 + 2 Wp + 2]; P0 and Wp are even
      q0 = P0;
      WL = (int)(P1 - P0) + 2 * g.Wp + 3;
      s2_half = __builtin_amdgcn_readfirstlane((WL + 1) >> 1);
      WS = 2 * s2_half;
    } else {
    // window = [first source pixel any tap reads, last one]: plain conv: consecutive pixels, one halo of Wp + 1 on either side;
    // UP: output rows 2r and 2r + 1 read the same source row, so the window holds whole source rows (first row's start .. last row's end)
    q0 = (UP ? P0 - (x_a >> 1) : P0) - (uint32_t)(g.Wp + 1);   // padded index of window pixel 0
    WL = WS = (int)((UP ? P1 - (x_b >> 1) + (uint32_t)p.iw - 1 : P1) - q0) + g.Wp + 2;  // window pixels this tile reads (<= WCAP)
    }
  }
  const int npc = __builtin_amdgcn_readfirstlane((WS + 7) >> 3);

  // ---- window fill: lane (pixel 8 pc + sr, physical chunk sp) of piece pc fetches logical chunk sp ^ key(pixel) ----
  int woff[PPW];  // byte offset of the lane's 16 bytes in slab 0, or -1: frame pixel / past the batch -> zero page
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int pc = i * NW + wave;
    const int j = 8 * pc + sr;
    const int chunk = sp ^ ((j >> 1) & 7);  // = src_chunk(sp, key_nat(j)), written out here and for the weight rows: four instantiations change registers otherwise
    bool ok;
    uint32_t pix;
    if constexpr (T2D && S2) {  // slot j = (wy, r): source row 2 t_y0 + wy, column 2 t_x0 + (r < 17 ? 2 r : 2 (r - 17) + 1)
      const int wy = j / 33, r = j - wy * 33;
      const int sy = 2 * (int)t_y0 + wy, sx = 2 * (int)t_x0 + (r < 17 ? 2 * r : 2 * (r - 17) + 1);
      ok = (j < WL2) & (sy < p.ih) & (sx < p.iw);  // the bottom row / right column past the image are the zero padding
      pix = (uint32_t)sy * (uint32_t)p.iw + (uint32_t)sx;
    } else if constexpr (T2D) {  // window pixel j = (wy, wx) of the (SH2 + 2) x PITCH2 block around the tile's source pixels
      const int wy = j / PITCH2, wx = j - wy * PITCH2;
      const int sy = (int)(UP ? t_y0 >> 1 : t_y0) - 1 + wy, sx = (int)(UP ? t_x0 >> 1 : t_x0) - 1 + wx;
      ok = (j < WL2) & (sy >= 0) & (sy < p.ih) & (sx >= 0) & (sx < p.iw);
      pix = (uint32_t)sy * (uint32_t)p.iw + (uint32_t)sx;  // inside the tile's image: its base is added as a 64-bit scalar (a_img)
    } else if constexpr (S2) {  // slot j: padded index q0 + 2 j (j < HALF) or q0 + 2 (j - HALF) + 1; the frame is row ih / columns >= iw
      const int jj = j < s2_half ? 2 * j : 2 * (j - s2_half) + 1;
      const uint32_t q = q0 + (uint32_t)jj;
      const uint32_t img = __umulhi(q, g.mul_sp);
      const uint32_t rem = q - img * (uint32_t)g.Sp;
      const uint32_t py = __umulhi(rem, g.mul_wp);
      const uint32_t px = rem - py * (uint32_t)g.Wp;
      ok = (img < (uint32_t)p.n) & (py < (uint32_t)p.ih) & (px < (uint32_t)p.iw) & (jj < WL);
      pix = (img * (uint32_t)p.ih + py) * (uint32_t)p.iw + px;
    } else {
      const uint32_t q = q0 + (uint32_t)j;
      const uint32_t img = __umulhi(q, g.mul_sp);
      const uint32_t rem = q - img * (uint32_t)g.Sp;
      const uint32_t py = __umulhi(rem, g.mul_wp);
      const uint32_t px = rem - py * (uint32_t)g.Wp;
      ok = (img < (uint32_t)p.n) & (py >= 1u) & (px >= 1u) & (j < WL);  // row 0 / column 0 of an image block are frame cells
      pix = (img * (uint32_t)p.ih + (py - 1)) * (uint32_t)p.iw + (px - 1);
    }
    woff[i] = ok ? (int)((pix * (uint32_t)p.cin + (uint32_t)chunk * 8u) * 2u) : -1;
  }
  // 2-D tiles: offsets are relative to the tile's image, so nothing here depends on the batch size (whether this kernel runs must be a
  // function of per-sample dimensions only: per-frame results are then identical whatever the number of frames per pass)
  const char* const a_img = (const char*)p.a + (T2D ? (int64_t)t_img * p.ih * p.iw * p.cin * 2 : (int64_t)0);
  auto fill_piece = [&](int i, int s, int wb) {  // i: compile-time after unrolling
    const int pc = i * NW + wave;
    if (pc < npc) {  // wave-uniform
      const char* const src = woff[i] >= 0 ? a_img + (int64_t)s * 128 + woff[i] : (const char*)g_zero_page;
      glds16_raw(src, lds_base_u32 + wb * WIN_BYTES + pc * 1024);
    }
  };
  auto fill_window = [&](int s, int wb) {
#pragma unroll
    for (int i = 0; i < PPW; ++i) fill_piece(i, s, wb);
  };

  // ---- weight stage: BN rows x 128 B of K-tile (tap t, slab s) = columns t * cin + 64 s ----
  const half_t* b_ptr[BPW];
#pragma unroll
  for (int i = 0; i < BPW; ++i) {
    const int row = 8 * (i * NW + wave) + sr;
    const int q = sp ^ ((row >> 1) & 7);
    int64_t n = n0 + row;
    if (n >= p.N) n = p.N - 1;
    b_ptr[i] = p.w + (PH ? (int64_t)ph * p.N * p.K : (int64_t)0) + n * p.K + q * 8;
  }
  auto stage_w = [&](int buf, int kcol) {
#pragma unroll
    for (int i = 0; i < BPW; ++i) {
      const int pc = i * NW + wave;
      if (NBP % NW == 0 || pc < NBP) glds16_raw(b_ptr[i] + kcol, lds_base_u32 + NWB * WIN_BYTES + buf * B_BYTES + pc * 1024);
    }
  };

  // ---- fragment addresses ----
  int b_off[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const int rb = wn * WN + fr;
    b_off[s2] = rb * 128 + (((4 * s2 + fg) ^ ((rb >> 1) & 7)) << 4);  // (frag_off, written out like the window's below: see there)
  }
  // window pixel of row (16 i + fr) of the wave's tile: plain conv at tap (0, 0), the tap shift ky * Wp + kx is a uniform scalar;
  // UP: at ky = 0 / 1 / 2 with kx = 1, plus the pixel's column parity (the kx shift is (xpar - 1, 0, xpar))
  int a_base[MI], a_rm[UP ? MI : 1], a_rp[UP ? MI : 1], a_xp[UP ? MI : 1];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    int ctr, yp, xp;  // window pixel under the centre tap; (UP) row / column parity of the output pixel
    if constexpr (T2D && S2) {
      ctr = 2 * (wm * (WM / 16) + i) * 33 + fr;  // slot of tap (0, 0): source row 2 x tile row, even column 2 fr
      yp = xp = 0;
    } else if constexpr (T2D) {
      const int row = wm * (WM / 16) + i;  // tile row = MFMA block
      ctr = UP ? ((row >> 1) + 1) * PITCH2 + (fr >> 1) + 1 : (row + 1) * PITCH2 + fr + 1;
      yp = row & 1;  // the tile's origin is even in both directions
      xp = fr & 1;
    } else {
      uint32_t m = row_m(i), yo, xo;
      if (m >= m_end) m = m_end - 1;
      ctr = (int)(pad_index(m, yo, xo) - q0);
      if constexpr (S2) ctr >>= 1;  // even padded index -> its slot
      yp = (int)(yo & 1);
      xp = (int)(xo & 1);
    }
    if constexpr (UP) {
      a_base[i] = ctr;
      a_rm[i] = ctr + (yp - 1) * pitch;
      a_rp[i] = ctr + yp * pitch;
      a_xp[i] = xp;
    } else {
      a_base[i] = S2 ? ctr : ctr - pitch - 1;
    }
  }

  const int nslab = p.cin / BK;
  fill_window(0, 0);
  stage_w(0, 0);
  // FP8: E8M0 scale bytes of this lane's weight rows (MFMA row fr of block j), four blocks per word (plain byte loads, retired below; this,
  // the pins and the tap's product are written out: as shared helpers they change 11 / 9 / 4 instantiations)
  constexpr int NSC = (NJ + 3) / 4;
  int wsc[FP8 ? NSC : 1];
  if constexpr (FP8) {
#pragma unroll
    for (int w = 0; w < NSC; ++w) wsc[w] = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      int64_t n = n0 + wn * WN + 16 * j + fr;
      if (n >= p.N) n = p.N - 1;
      wsc[j >> 2] |= (int)p.w_exp[n] << (8 * (j & 3));
    }
  }

  f32x4 acc[MI][NJ];
  if (!PH && p.residual) {  // the residual tile goes straight into the accumulators (written out: as a shared helper 21 instantiations change registers)
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      int64_t m = row_m(i);
      if (m >= m_end) m = m_end - 1;
      const float* rp = p.residual + m * p.ldr;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        int64_t f = n0 + wn * WN + 16 * j + 4 * fg;
        if (f > p.N - 4) f = p.N - 4;
        acc[i][j] = *(const f32x4*)(rp + f);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  drain_barrier();
  // retire the residual loads for hipcc's wait bookkeeping HERE: a load still "possibly pending" at the loop header gets a literal
  // vmcnt in front of its first use in every iteration, and that literal would also drain the LDS-DMA the compiler cannot see
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(acc[i][j]));
  if constexpr (FP8) {
#pragma unroll
    for (int w = 0; w < NSC; ++w) asm volatile("" : "+v"(wsc[w]));
  }

  int cur = 0;  // weight stage of the K-tile being computed
  for (int s = 0; s < nslab; ++s) {
    const char* const win = lds_win + (DBW ? (s & 1) * WIN_BYTES : 0);
    const bool more = s + 1 < nslab;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t < NT - 1) stage_w(cur ^ 1, (t + 1) * p.cin + BK * s);
      else if (more) stage_w(cur ^ 1, BK * (s + 1));
      if constexpr (DBW && !PH) {  // the next slab's window, one piece per wave and tap, into the other buffer
        if (more && t < PPW) fill_piece(t, s + 1, (s + 1) & 1);
      }
      if constexpr (DBW && PH) {  // four taps: two pieces per wave and tap
        static_assert(!PH || PPW <= 2 * NT, "phase mode: two window pieces per wave and tap");
        if (more && 2 * t < PPW) fill_piece(2 * t, s + 1, (s + 1) & 1);
        if (more && 2 * t + 1 < PPW) fill_piece(2 * t + 1, s + 1, (s + 1) & 1);
      }
      const char* const tb = lds_b + cur * B_BYTES;
      int toff = S2 ? (t / 3) * (T2D ? 33 : g.Wp >> 1) + ((t % 3) & 1) * s2_half + ((t % 3) >> 1) : UP ? 0 : PH ? ((t >> 1) + (ph >> 1)) * pitch + (t & 1) + (ph & 1) : (t / 3) * pitch + (t % 3);
      asm volatile("" : "+s"(toff));  // opaque: the nine taps' fragment addresses are formed here, not hoisted out of the slab loop (45 registers)
      // fragment reads + MFMAs of the tap.  FIRST: every fragment read is ISSUED before the first MFMA (hipcc otherwise re-uses one
      // register quad for the second k-step's window fragments and waits for each read right in front of the five MFMAs that need it:
      // ~100 exposed cycles four times per tap); the MFMAs then start behind counted lgkmcnt waits as the fragments arrive in order.
      // Measured (profiles/r04_kconvwin_frags_first.log): +1.5 ... 9 % on the 4-wave family (two independent workgroups per CU), -8 ... 10 %
      // on the 8-wave family, whose waves would all burst their 18 reads right behind the shared barrier: it keeps hipcc's interleaving.
      const auto compute_tap = [&](auto first_c) {
        constexpr bool FIRST = decltype(first_c)::value;
        half8_t af[2][MI], bf[2][NJ];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          int j;
          if constexpr (UP) {
            const int ky = t / 3, kx = t % 3;  // compile-time after unrolling
            j = (ky == 0 ? a_rm[i] : ky == 1 ? a_base[i] : a_rp[i]) + (kx == 0 ? a_xp[i] - 1 : kx == 1 ? 0 : a_xp[i]) + toff;
          } else {
            j = a_base[i] + toff;
          }
          const int addr = j * 128 + ((fg ^ ((j >> 1) & 7)) << 4);  // (frag_off written out: the 256-row phase kernel's tap loop loses an s_nop otherwise, and the 72 x 72, 960 -> 320 conv measured 0.8 % slower)
          af[0][i] = *(const half8_t*)(win + addr);
          af[1][i] = *(const half8_t*)(win + (addr ^ 64));
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int j = 0; j < NJ; ++j) bf[s2][j] = *(const half8_t*)(tb + b_off[s2] + j * 2048);
        if constexpr (FIRST) __builtin_amdgcn_sched_barrier(0);
        if constexpr (FP8) {
#pragma unroll
          for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = mfma_f8(j, bf[0][j], bf[1][j], af[0][i], af[1][i], acc[i][j], wsc[j >> 2]);
        } else {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[s2][j], af[s2][i], acc[i][j], 0, 0, 0);
        }
      };
      if constexpr (NW == 4 && !FP8) {
        compute_tap(std::true_type{});
      } else {  // (giving the two wave groups of the 8-wave workgroup different orders under a wave-uniform branch spills 139+ registers)
        compute_tap(std::false_type{});
      }
      if constexpr (FP8) {  // pin the tap's MFMAs in front of its barrier (the same pin on the f16 8-wave family: conv class +0.3 ms, not done): hipcc otherwise sinks all nine taps' scaled MFMAs behind the last
                            // barrier of the slab and parks their fragments in scratch (2 KB; seen in the ISA)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(acc[i][j]));
      }
      if constexpr (!DBW) {
        if (t == NT - 1 && more) {  // every wave has read the last tap's fragments: the window is free for the next slab
          lds_barrier();
          fill_window(s + 1, 0);
        }
      }
      drain_barrier();
      cur ^= 1;
    }
  }

  // ---- epilogue (gemm.hip's plain one): lane holds features f .. f+3 (rows of D) of pixel m (column of D) ----
  f32x4 bj[NJ];
  int fj[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    int64_t f = n0 + wn * WN + 16 * j + 4 * fg;
    if (f > p.N - 4) f = p.N - 4;  // clamp loads; stores are guarded below
    fj[j] = (int)f;
    bj[j] = p.bias ? first_read(*(const f32x4*)(p.bias + f)) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int64_t m = row_m(i);
    const int64_t mc = m < m_end ? m : m_end - 1;
    int64_t mo = m;  // output row; PH: source pixel (img, i, j) -> output pixel (img, 2i + py, 2j + px)
    if constexpr (PH && T2D) {  // the tile knows its image and origin: no division (the multiply-high ones hold for linear launches only)
      const uint32_t yi = t_y0 + (uint32_t)(wm * (WM / 16) + i), xj = t_x0 + (uint32_t)fr;
      mo = (int64_t)t_img * (4 * g.hw) + (int64_t)(2 * yi + (uint32_t)(ph >> 1)) * (2 * g.ow) + 2 * xj + (uint32_t)(ph & 1);
    } else if constexpr (PH) {
      const uint32_t img = __umulhi((uint32_t)mc, g.mul_hw), rem = (uint32_t)mc - img * (uint32_t)g.hw;
      const uint32_t yi = __umulhi(rem, g.mul_iw), xj = rem - yi * (uint32_t)g.ow;
      mo = (int64_t)img * (4 * g.hw) + (int64_t)(2 * yi + (uint32_t)(ph >> 1)) * (2 * g.ow) + 2 * xj + (uint32_t)(ph & 1);
    }
    f32x4 v[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) v[j] = acc[i][j] + bj[j];
    if (!PH && p.row_add) {
      const float* rp = p.row_add + (mc / p.rows_per_group) * p.ldra;
#pragma unroll
      for (int j = 0; j < NJ; ++j) v[j] += first_read(*(const f32x4*)(rp + fj[j]));
    }
    if constexpr (STATS) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = v[j];  // the statistics pass reads the final values
    }
    const bool row_ok = m < m_end;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int64_t f = n0 + wn * WN + 16 * j + 4 * fg;
      if (!row_ok || f >= p.N) continue;
      if (p.out_f32) *(f32x4*)(p.out_f32 + mo * p.ldo32 + f) = v[j];
      if (!PH && p.out_f16) *(half4_t*)(p.out_f16 + m * p.ldo16 + f) = to_f16x4(v[j]);
    }
    if constexpr (O8) {
      // e4m3 output (saturating, RNE; gemm.hip's GEGLU out_f8): a lane holds 4 features of block j, its partner lane ^ 16 the next 4.  One
      // swizzle per pair of blocks hands each lane the partner's quad, so that every lane stores 8 consecutive features in one 8-byte store:
      // even fg lanes of block j, odd fg lanes of block j + 1
      static_assert(NJ % 2 == 0, "out_f8: blocks in pairs");
      if (p.out_f8) {
        typedef int v2i_t __attribute__((ext_vector_type(2)));
        const bool odd = (fg & 1) != 0;
#pragma unroll
        for (int j = 0; j < NJ; j += 2) {
          const int q0 = pack_fp8x4(v[j][0], v[j][1], v[j][2], v[j][3]);
          const int q1 = pack_fp8x4(v[j + 1][0], v[j + 1][1], v[j + 1][2], v[j + 1][3]);
          const int got = __builtin_amdgcn_ds_swizzle(odd ? q0 : q1, 0x401F);  // bit-mask mode: and 0x1f, xor 0x10 -> lane ^ 16
          const int64_t f = n0 + wn * WN + 16 * (odd ? j + 1 : j) + 4 * (fg & 2);
          if (row_ok && f + 8 <= p.N) *(v2i_t*)(p.out_f8 + m * p.ldo8 + f) = odd ? v2i_t{got, q1} : v2i_t{q0, got};
        }
      }
    }
  }
  if constexpr (STATS) {
    if (p.ch_stats != nullptr) {  // per 64-row block and channel: sum and sum of squares (gemm.hip, same association; written out: as a shared helper 14 instantiations change)
      // block number: linear tiles: 64 consecutive rows of the tensor; 2-D tiles: the wave's 4 tile rows x 16 pixels, numbered inside the image
      const int64_t mw = (int64_t)m0 + wm * WM;
      // PH: the wave's 64 source pixels are 64 OUTPUT pixels of one phase and one image (hw % 64 == 0): block 4 * (source block) + phase,
      // so the hw_out / 64 blocks of image i fill [i hw_out / 64, (i + 1) hw_out / 64), each written once
      static_assert(SEVA_CH_STATS_ROWS == 64, "a block of ch_stats is the wave's 64 rows");
      const int64_t sblk = T2D ? (int64_t)t_img * (g.hw >> 6) + (int64_t)t_k * (BM / 64) + wm : mw >> 6;
      const int64_t blk = PH ? 4 * sblk + ph : sblk;
      float* const sp_ = p.ch_stats + blk * 2 * p.N;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        f32x4 ssum = {0.f, 0.f, 0.f, 0.f}, qsum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const f32x4 vm = (T2D || mw + 16 * i + fr < m_end) ? acc[i][j] : f32x4{0.f, 0.f, 0.f, 0.f};  // rows past the tile contribute nothing
          ssum += vm;
          qsum += vm * acc[i][j];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ssum[r] = row16_sum(ssum[r]);
          qsum[r] = row16_sum(qsum[r]);
        }
        const int64_t f = n0 + wn * WN + 16 * j + 4 * fg;
        if (fr == 0 && (T2D || mw < m_end) && f < p.N) {
          *(f32x4*)(sp_ + f) = ssum;
          *(f32x4*)(sp_ + p.N + f) = qsum;
        }
      }
    }
  }
}


// Launches one row of the instantiation table (gemm_plan.h: SEVA_WIN_KERNELS) over the plan's ranges of whole images: outputs, residual,
// row_add and statistics move by whole images (the plan keeps a range's first row on a row_add group boundary and on a 64-row block).
template <int BM, int BN, int NW, int WCAP, bool DBW, bool STATS, bool UP, int TW, bool FP8, bool O8, bool S2, bool PH>
int launch_win(const GemmArgs& a, const seva_plan::WinPlan& w, hipStream_t s) {
  constexpr int lds = (DBW ? 2 : 1) * WCAP * 128 + 2 * BN * 128;
  static_assert(lds <= 160 * 1024, "LDS per workgroup");
  static std::atomic<uint64_t> attr_devs{0};
  seva_max_dynamic_lds_once(attr_devs, lds, {(const void*)conv_win_kernel<BM, BN, NW, WCAP, DBW, STATS, UP, TW, FP8, O8, S2, PH>});
  const seva_plan::WinGeom& pg = w.geom;
  ConvWinGeom g{};
  g.mul_hw = pg.mul_hw; g.mul_iw = pg.mul_iw; g.mul_sp = pg.mul_sp; g.mul_wp = pg.mul_wp;
  g.Wp = pg.Wp; g.Sp = pg.Sp; g.hw = pg.hw; g.ow = pg.ow;
  g.tiles_n = pg.tiles_n;
  g.n_lin = pg.n_lin;
  int64_t i0 = 0;  // first image of the range
  for (int r = 0; r < w.n_ranges(); ++r) {
    const seva_plan::WinTiling& t = w.range(r);
    const int64_t r0 = i0 * g.hw;
    GemmArgs c = a;
    c.n = t.n;
    c.M = (int64_t)t.n * g.hw;
    c.a = a.a + i0 * a.ih * a.iw * a.cin;
    if (c.residual) c.residual += r0 * a.ldr;
    if (c.out_f32) c.out_f32 += r0 * (PH ? 4 : 1) * a.ldo32;  // (PH: r0 counts source pixels, four output rows each)
    if (c.out_f16) c.out_f16 += r0 * a.ldo16;
    if (c.out_f8) c.out_f8 += r0 * a.ldo8;
    if (c.row_add) c.row_add += (r0 / a.rows_per_group) * a.ldra;
    if (c.ch_stats) c.ch_stats += (r0 / 64) * (PH ? 4 : 1) * 2 * a.N;
    g.tpi = t.tpi;
    g.tiles_m = t.tiles_m;
    const int64_t nb = (int64_t)g.tiles_m * g.tiles_n * (PH ? 4 : 1);  // PH: one workgroup per tile and phase
    if (nb <= 0 || nb > 0x7fffffff) {
      seva_set_error("conv_win: bad grid %lld", (long long)nb);
      return SEVA_ERR_ARG;
    }
    hipLaunchKernelGGL((conv_win_kernel<BM, BN, NW, WCAP, DBW, STATS, UP, TW, FP8, O8, S2, PH>), dim3((unsigned)nb), dim3(64 * NW), lds, s, c, g);
    const int rc = seva_check_launch("conv_win_kernel");
    if (rc != 0) return rc;
    i0 += t.n;
  }
  return 0;
}

}  // namespace

int seva_conv_win_launch(const GemmArgs& a0, const seva_plan::WinPlan& w, hipStream_t s) {
  const seva_plan::WinCfg none{};
  const seva_plan::WinCfg& c = w.win >= 0 ? w.cand[w.win] : none;
  GemmArgs a = a0;  // the kernel's view (the phase modes: a plain conv over the SOURCE image, one launch row per source pixel)
  a.oh = w.problem.oh;
  a.ow = w.problem.ow;
  a.M = w.problem.M;
#define SEVA_LAUNCH_ROW(NAME, BM, BN, NW, WCAP, DBW, STATS, UP, TW, FP8, O8, S2, PH)                               \
  if (seva_plan::same_kernel(c, seva_plan::WinCfg{BM, BN, NW, WCAP, DBW, STATS, UP, TW, FP8, O8, S2, PH})) {    \
    g_seva_last_plan = NAME;                                                                                       \
    return launch_win<BM, BN, NW, WCAP, DBW, STATS, UP, TW, FP8, O8, S2, PH>(a, w, s);                             \
  }
  SEVA_WIN_KERNELS(SEVA_LAUNCH_ROW)
#undef SEVA_LAUNCH_ROW
  seva_set_error("conv_win: internal error: no conv_win_kernel<%d, %d, %d, %d> instantiation with dbw %d stats %d up %d tw %d fp8 %d o8 %d s2 %d "
                 "ph %d (candidate %d of %d)", c.bm, c.bn, c.nw, c.wcap, c.dbw, c.stats, c.up, c.tw, c.fp8, c.o8, c.s2, c.ph, w.win, w.n_cand);
  return SEVA_ERR_ARG;
}
