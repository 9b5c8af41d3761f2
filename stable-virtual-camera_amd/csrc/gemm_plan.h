// Which kernel instantiation and which tiling serve a seva_gemm_desc: the dispatch policy of seva_gemm_f16 / seva_gemm_f16_split_out /
// seva_gemm_fp8 as a pure function, plan(), of the VALIDATED descriptor, the knobs and the variant.  It reads problem dimensions,
// null-ness of pointers and flags only, launches nothing and includes no HIP header: gemm.hip / conv_win.hip launch what it returns,
// gemm_plan_dump.cpp prints it (tests/test_gemm_plan_cpu.py checks the policy without a GPU).
//
// The project's bit-equality promises (frame slicing, the CFG split over ranks, sharded == single-process) rest on this file: whether
// a sample is computed by the window kernel or the per-tap gather, split-K or not, on linear or 2-D window tiles, and in ranges of how
// many images (n_lin) depends on PER-SAMPLE dimensions only.  Tile height, 4 vs 8 waves and the A-in-registers variant may follow the
// batch: they are bitwise equal to each other (tests/test_ops_gpu.py, tests/test_gemm_contract_gpu.py).
#pragma once

#include <stdint.h>

#include <initializer_list>
#include <numeric>

#include "../../include/seva_hip.h"
#include "seva_knobs.h"

namespace seva_plan {

constexpr int BK = 64;  // fp16 elements per K-tile -> 128-byte LDS rows

enum Variant { F16 = 0, F16_SPLIT_OUT = 1, FP8 = 2 };

// ---------------------------------------------------------------------------------------------------------------------------------
// instantiation tables: every gemm_kernel / conv_win_kernel instantiation of the library is one row, written once.  gemm.hip and
// conv_win.hip expand the rows into their launchers, the arrays below show them to the planner's consumers.
// ---------------------------------------------------------------------------------------------------------------------------------

// gemm_kernel<BM, BN, MODE, EPI, DBGK, PAIRED, ASTAT, FP8, SPLITK, NW, SPLIT16> (gemm.hip).  MODE 0 GEMM, 1 conv gather, 2 conv gather
// of the nearest-2x upsampled image, 3 conv gather + folded second operand; EPI 1 = GEGLU.  A row stands for the production kernel
// (DBGK = false) and, where has_dbgk() holds, for its ablation twin (DBGK = true) as well.
struct GemmCfg {
  int bm, bn, mode, epi;
  bool paired, astat, fp8, splitk;
  int nw;
  bool split16;
  bool dbgk;  // not a table column: see has_dbgk()
};
// the ablation instantiation only exists for the staged-A f16 kernels
constexpr bool has_dbgk(const GemmCfg& c) { return !c.astat && !c.fp8 && !c.splitk && c.nw == 4 && !c.split16; }

//   name                              BM   BN  MODE EPI PAIRED ASTAT  FP8    SPLITK NW SPLIT16
#define SEVA_GEMM_KERNELS(X)                                                                  \
  X("gemm 64x128 f32",                 64, 128, 0, 0, false, false, false, false, 4, false)   \
  X("gemm 64x128 f16-only",            64, 128, 0, 0, true,  false, false, false, 4, false)   \
  X("gemm 64x128 e4m3 f32",            64, 128, 0, 0, false, false, true,  false, 4, false)   \
  X("gemm 64x128 e4m3 f16-only",       64, 128, 0, 0, true,  false, true,  false, 4, false)   \
  X("gemm 64x160 f32",                 64, 160, 0, 0, false, false, false, false, 4, false)   \
  X("gemm 64x160 f16-only",            64, 160, 0, 0, true,  false, false, false, 4, false)   \
  X("gemm 64x160 e4m3 f32",            64, 160, 0, 0, false, false, true,  false, 4, false)   \
  X("gemm 64x160 e4m3 f16-only",       64, 160, 0, 0, true,  false, true,  false, 4, false)   \
  X("gemm 128x32 f32 narrow",         128,  32, 0, 0, false, false, false, false, 4, false)   \
  X("gemm 128x128 f32",               128, 128, 0, 0, false, false, false, false, 4, false)   \
  X("gemm 128x128 f16-only",          128, 128, 0, 0, true,  false, false, false, 4, false)   \
  X("gemm 128x128 f16-only A-in-regs",128, 128, 0, 0, true,  true,  false, false, 4, false)   \
  X("gemm 128x128 e4m3 f32",          128, 128, 0, 0, false, false, true,  false, 4, false)   \
  X("gemm 128x128 e4m3 f16-only",     128, 128, 0, 0, true,  false, true,  false, 4, false)   \
  X("gemm 128x128 split-out",         128, 128, 0, 0, false, false, false, false, 4, true)    \
  X("gemm 128x160 f32",               128, 160, 0, 0, false, false, false, false, 4, false)   \
  X("gemm 128x160 f16-only",          128, 160, 0, 0, true,  false, false, false, 4, false)   \
  X("gemm 128x160 f16-only A-in-regs",128, 160, 0, 0, true,  true,  false, false, 4, false)   \
  X("gemm 128x160 split-out",         128, 160, 0, 0, false, false, false, false, 4, true)    \
  X("gemm 160x160 f32",               160, 160, 0, 0, false, false, false, false, 4, false)   \
  X("geglu 64x128",                    64, 128, 0, 1, true,  false, false, false, 4, false)   \
  X("geglu 64x128 e4m3",               64, 128, 0, 1, true,  false, true,  false, 4, false)   \
  X("geglu 128x128",                  128, 128, 0, 1, true,  false, false, false, 4, false)   \
  X("geglu 128x128 A-in-regs",        128, 128, 0, 1, true,  true,  false, false, 4, false)   \
  X("geglu 128x128 e4m3",             128, 128, 0, 1, true,  false, true,  false, 4, false)   \
  X("geglu 128x128 split-out",        128, 128, 0, 1, true,  false, false, false, 4, true)    \
  X("geglu 160x128",                  160, 128, 0, 1, true,  false, false, false, 4, false)   \
  X("conv gather 64x128",              64, 128, 1, 0, false, false, false, false, 4, false)   \
  X("conv gather 64x128 e4m3",         64, 128, 1, 0, false, false, true,  false, 4, false)   \
  X("conv gather 64x160",              64, 160, 1, 0, false, false, false, false, 4, false)   \
  X("conv gather 64x160 e4m3",         64, 160, 1, 0, false, false, true,  false, 4, false)   \
  X("conv gather 128x32 narrow",      128,  32, 1, 0, false, false, false, false, 4, false)   \
  X("conv gather 128x128",            128, 128, 1, 0, false, false, false, false, 4, false)   \
  X("conv gather 128x128 e4m3",       128, 128, 1, 0, false, false, true,  false, 4, false)   \
  X("conv gather 128x128 split-K",    128, 128, 1, 0, false, false, false, true,  4, false)   \
  X("conv gather 128x160",            128, 160, 1, 0, false, false, false, false, 4, false)   \
  X("conv gather 128x160 split-K",    128, 160, 1, 0, false, false, false, true,  4, false)   \
  X("conv gather 160x160",            160, 160, 1, 0, false, false, false, false, 4, false)   \
  X("conv gather upsample 64x128",     64, 128, 2, 0, false, false, false, false, 4, false)   \
  X("conv gather upsample 64x160",     64, 160, 2, 0, false, false, false, false, 4, false)   \
  X("conv gather upsample 128x32",    128,  32, 2, 0, false, false, false, false, 4, false)   \
  X("conv gather upsample 128x128",   128, 128, 2, 0, false, false, false, false, 4, false)   \
  X("conv gather upsample 128x160",   128, 160, 2, 0, false, false, false, false, 4, false)   \
  X("conv gather + a2 128x128",       128, 128, 3, 0, false, false, false, false, 4, false)   \
  X("conv gather + a2 128x160",       128, 160, 3, 0, false, false, false, false, 4, false)   \
  X("conv gather + a2 160x160",       160, 160, 3, 0, false, false, false, false, 4, false)

// conv_win_kernel<BM, BN, NW, WCAP, DBW, STATS, UP, TW, FP8, O8, S2, PH> (conv_win.hip).  WCAP: window capacity in pixels; DBW: window
// double-buffered (the 8-wave 256-row tile); STATS: the instantiation CAN emit statistics; UP: fused nearest-2x upsample; TW = 16: 2-D
// tiles; O8: e4m3 output epilogue; S2: stride 2, bottom / right padding; PH: one 2x2 phase conv of the upsample per workgroup.
struct WinCfg {
  int bm, bn, nw, wcap;
  bool dbw, stats, up;
  int tw;
  bool fp8, o8, s2, ph;
  // how the planner spells a candidate: win4(...) / win8(...) plus the properties that differ from the plain f16 linear kernel
  constexpr WinCfg upsampled() const { WinCfg c = *this; c.up = true; return c; }
  constexpr WinCfg tiles2d() const { WinCfg c = *this; c.tw = 16; return c; }
  constexpr WinCfg e4m3() const { WinCfg c = *this; c.fp8 = true; return c; }
  constexpr WinCfg out8() const { WinCfg c = *this; c.o8 = true; return c; }
  constexpr WinCfg stride2() const { WinCfg c = *this; c.s2 = true; return c; }
  constexpr WinCfg phases() const { WinCfg c = *this; c.ph = true; return c; }
};
// two 4-wave workgroups per CU, window single-buffered
constexpr WinCfg win4(int bm, int bn, int wcap, bool stats) { return WinCfg{bm, bn, 4, wcap, false, stats, false, 0, false, false, false, false}; }
// one 8-wave workgroup per CU on a 256-row tile, window double-buffered
constexpr WinCfg win8(int bn, int wcap, bool stats) { return WinCfg{256, bn, 8, wcap, true, stats, false, 0, false, false, false, false}; }

//   name                                        BM   BN NW WCAP DBW    STATS  UP     TW  FP8    O8     S2     PH
#define SEVA_WIN_KERNELS(X)                                                                                        \
  X("win 4-wave 160x32 linear narrow",          160,  32, 4, 320, false, false, false,  0, false, false, false, false) \
  X("win 4-wave 128x32 2-D narrow",             128,  32, 4, 184, false, false, false, 16, false, false, false, false) \
  X("win 4-wave 160x160 linear",                160, 160, 4, 320, false, false, false,  0, false, false, false, false) \
  X("win 4-wave 128x160 linear stats",          128, 160, 4, 288, false, true,  false,  0, false, false, false, false) \
  X("win 8-wave 256x160 linear stats",          256, 160, 8, 416, true,  true,  false,  0, false, false, false, false) \
  X("win 4-wave 128x160 linear upsample",       128, 160, 4, 288, false, true,  true,   0, false, false, false, false) \
  X("win 8-wave 256x160 linear upsample",       256, 160, 8, 416, true,  true,  true,   0, false, false, false, false) \
  X("win 4-wave 128x128 linear stats",          128, 128, 4, 288, false, true,  false,  0, false, false, false, false) \
  X("win 4-wave 128x128 2-D stats",             128, 128, 4, 184, false, true,  false, 16, false, false, false, false) \
  X("win 8-wave 256x128 linear stats",          256, 128, 8, 416, true,  true,  false,  0, false, false, false, false) \
  X("win 8-wave 256x128 2-D stats",             256, 128, 8, 328, true,  true,  false, 16, false, false, false, false) \
  X("win 4-wave 128x128 linear upsample",       128, 128, 4, 288, false, true,  true,   0, false, false, false, false) \
  X("win 4-wave 128x128 2-D upsample",          128, 128, 4,  64, false, true,  true,  16, false, false, false, false) \
  X("win 8-wave 256x128 linear upsample",       256, 128, 8, 416, true,  true,  true,   0, false, false, false, false) \
  X("win 8-wave 256x128 2-D upsample",          256, 128, 8, 104, true,  true,  true,  16, false, false, false, false) \
  X("win e4m3 4-wave 128x128 linear stats",     128, 128, 4, 288, false, true,  false,  0, true,  false, false, false) \
  X("win e4m3 4-wave 128x128 2-D stats",        128, 128, 4, 184, false, true,  false, 16, true,  false, false, false) \
  X("win e4m3 8-wave 256x128 linear stats",     256, 128, 8, 416, true,  true,  false,  0, true,  false, false, false) \
  X("win e4m3 8-wave 256x128 2-D stats",        256, 128, 8, 328, true,  true,  false, 16, true,  false, false, false) \
  X("win e4m3 4-wave 128x128 linear upsample",  128, 128, 4, 288, false, true,  true,   0, true,  false, false, false) \
  X("win e4m3 4-wave 128x128 2-D upsample",     128, 128, 4,  64, false, true,  true,  16, true,  false, false, false) \
  X("win e4m3 8-wave 256x128 linear upsample",  256, 128, 8, 416, true,  true,  true,   0, true,  false, false, false) \
  X("win e4m3 8-wave 256x128 2-D upsample",     256, 128, 8, 104, true,  true,  true,  16, true,  false, false, false) \
  X("win e4m3 4-wave 128x128 linear out_f8",    128, 128, 4, 288, false, true,  false,  0, true,  true,  false, false) \
  X("win e4m3 4-wave 128x128 2-D out_f8",       128, 128, 4, 184, false, true,  false, 16, true,  true,  false, false) \
  X("win e4m3 8-wave 256x128 linear out_f8",    256, 128, 8, 416, true,  true,  false,  0, true,  true,  false, false) \
  X("win e4m3 8-wave 256x128 2-D out_f8",       256, 128, 8, 328, true,  true,  false, 16, true,  true,  false, false) \
  X("win e4m3 4-wave 128x128 linear stride 2",  128, 128, 4, 864, false, true,  false,  0, true,  false, true,  false) \
  X("win e4m3 4-wave 128x128 2-D stride 2",     128, 128, 4, 568, false, true,  false, 16, true,  false, true,  false) \
  X("win phases 4-wave 160x160 linear",         160, 160, 4, 320, false, false, false,  0, false, false, false, true)  \
  X("win phases 8-wave 256x160 linear",         256, 160, 8, 416, true,  false, false,  0, false, false, false, true)  \
  X("win phases 4-wave 128x128 linear stats",   128, 128, 4, 288, false, true,  false,  0, false, false, false, true)  \
  X("win phases 4-wave 128x128 2-D stats",      128, 128, 4, 184, false, true,  false, 16, false, false, false, true)  \
  X("win phases 8-wave 256x128 linear stats",   256, 128, 8, 416, true,  true,  false,  0, false, false, false, true)  \
  X("win phases 8-wave 256x128 2-D stats",      256, 128, 8, 328, true,  true,  false, 16, false, false, false, true)

struct GemmRow { const char* name; GemmCfg cfg; };
struct WinRow { const char* name; WinCfg cfg; };
#define SEVA_ROW(NAME, BM, BN, MODE, EPI, PAIRED, ASTAT, FP8_, SPLITK, NW, SPLIT16) {NAME, {BM, BN, MODE, EPI, PAIRED, ASTAT, FP8_, SPLITK, NW, SPLIT16, false}},
constexpr GemmRow kGemmKernels[] = {SEVA_GEMM_KERNELS(SEVA_ROW)};
#undef SEVA_ROW
#define SEVA_ROW(NAME, BM, BN, NW, WCAP, DBW, STATS, UP, TW, FP8_, O8, S2, PH) {NAME, {BM, BN, NW, WCAP, DBW, STATS, UP, TW, FP8_, O8, S2, PH}},
constexpr WinRow kWinKernels[] = {SEVA_WIN_KERNELS(SEVA_ROW)};
#undef SEVA_ROW
constexpr int kNumGemmKernels = (int)(sizeof(kGemmKernels) / sizeof(kGemmKernels[0]));
constexpr int kNumWinKernels = (int)(sizeof(kWinKernels) / sizeof(kWinKernels[0]));

// a plan's configuration against a row (the ablation twin matches the row that has one)
constexpr bool same_kernel(const GemmCfg& p, const GemmCfg& r) {
  return p.bm == r.bm && p.bn == r.bn && p.mode == r.mode && p.epi == r.epi && p.paired == r.paired && p.astat == r.astat && p.fp8 == r.fp8 &&
         p.splitk == r.splitk && p.nw == r.nw && p.split16 == r.split16 && (!p.dbgk || has_dbgk(r));
}
constexpr bool same_kernel(const WinCfg& p, const WinCfg& r) {
  return p.bm == r.bm && p.bn == r.bn && p.nw == r.nw && p.wcap == r.wcap && p.dbw == r.dbw && p.stats == r.stats && p.up == r.up && p.tw == r.tw &&
         p.fp8 == r.fp8 && p.o8 == r.o8 && p.s2 == r.s2 && p.ph == r.ph;
}
// index of the row a configuration names, -1 if none (an internal error for a launcher)
inline int find_row(const GemmCfg& c) {
  for (int i = 0; i < kNumGemmKernels; ++i)
    if (same_kernel(c, kGemmKernels[i].cfg)) return i;
  return -1;
}
inline int find_row(const WinCfg& c) {
  for (int i = 0; i < kNumWinKernels; ++i)
    if (same_kernel(c, kWinKernels[i].cfg)) return i;
  return -1;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// "no benchmark knob forces anything": one predicate per distinct meaning
// ---------------------------------------------------------------------------------------------------------------------------------

// an ablation run (SEVA_GEMM_DBG / SEVA_GEMM_STAGGER set, 0 included): everything takes the staged-A kernels that have an ablation twin
inline bool ablation_run(const SevaKnobs& k) { return k.gemm_dbg >= 0 || k.gemm_stagger >= 0; }
// the A-in-registers variant (knob gemm_astat = 0 disables it; it has no ablation twin)
inline bool astat_allowed(const SevaKnobs& k) { return k.gemm_astat != 0 && !ablation_run(k); }
// nothing forces the tile HEIGHT: split-K (128-row tiles) and the 160-row GEGLU tiles may be chosen.  gemm_bn / gemm_chunks do not
// matter here: split-K follows a forced width, and both kernels take a forced chunk count.
inline bool tile_height_free(const SevaKnobs& k) { return k.gemm_bm <= 0 && !ablation_run(k); }
// nothing forces the tile SHAPE or the schedule: the f16 window kernel and the 160 x 160 tiles (fixed shapes, own schedules) may be
// chosen.  Differs from tile_height_free by gemm_bn and gemm_chunks.
inline bool tile_shape_free(const SevaKnobs& k) { return k.gemm_bm <= 0 && k.gemm_bn <= 0 && k.gemm_chunks <= 0 && !ablation_run(k); }
// the e4m3 window kernel may be chosen.  Differs from tile_shape_free in two ways: gemm_stagger is NOT looked at (the e4m3 kernels have
// no ablation twin, so a stagger run changes nothing for them), and the conv_win = 0 knob is part of it because the e4m3 errors for
// convs that only the window kernel runs are worded around this condition.
inline bool fp8_window_allowed(const SevaKnobs& k) {
  return k.conv_win != 0 && k.gemm_dbg < 0 && k.gemm_bm <= 0 && k.gemm_bn <= 0 && k.gemm_chunks <= 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// window kernel: geometry, candidates, tiling
// ---------------------------------------------------------------------------------------------------------------------------------

inline uint32_t magic_u32(uint32_t d) { return (uint32_t)(0x100000000ull / d) + 1u; }

// the numbers conv_win_kernel indexes a launch with (its ConvWinGeom), but tiles_m / tpi, which belong to a range (WinTiling)
struct WinGeom {
  uint32_t mul_hw, mul_iw, mul_sp, mul_wp;  // floor(2^32 / d) + 1: x / d == mulhi(x, mul) over the launch's range of x
  int32_t Wp, Sp, hw;                       // hw = OUTPUT pixels per image; mul_iw divides by the OUTPUT width ow
  int32_t ow;
  int32_t tiles_n;
  int32_t n_lin;  // images per launch of the linear tiles (31-bit offsets, exact multiply-high divisions); 0 = not even one
};

// The conv as the window kernel sees it (the GemmArgs fields of the launch): cin and K count 2-byte units (e4m3: pairs of elements); the
// phase modes put the SOURCE image into oh / ow / M.
struct WinProblem {
  int64_t M, N, K;
  int32_t n, ih, iw, cin, oh, ow, stride, upsample, pad_lo;
  int64_t rows_per_group;
  bool ch_stats, row_add, out_f8, w_exp, a2, sk_ws;
};

// Geometry of a launch (a.oh / a.ow: the image the kernel's M rows index).  false = the window kernel does not apply
inline bool win_geometry(const WinProblem& a, bool s2, WinGeom& g) {
  g = WinGeom{};
  // 31-bit byte offsets into ONE image.  First: with cin >= 64 it bounds ih * iw below 2^24, so the int products below cannot overflow.
  if ((uint64_t)a.ih * a.iw * a.cin * 2 >= (1ull << 31)) return false;
  g.Wp = a.iw + 1;             // padded SOURCE space (UP: the image before the nearest-2x upsample)
  if (s2) g.Wp += g.Wp & 1;    // S2: frame columns on the right only, as many as make the row pitch even (parity of P = parity of x)
  g.Sp = (a.ih + 1) * g.Wp;
  g.hw = a.oh * a.ow;
  g.ow = a.ow;
  // GroupNorm statistics are 64-row blocks of the whole tensor: only where a block cannot straddle two images (the consumer refuses other
  // statistics anyway), for every batch size
  if (a.ch_stats && g.hw % SEVA_CH_STATS_ROWS != 0) return false;
  // exactness of the multiply-high divisions of the LINEAR tiles (2-D tiles divide by constants
  // only): mulhi(x, floor(2^32 / d) + 1) == x / d for every x with x * e < 2^32, e = (floor(2^32 / d) + 1) * d - 2^32 in (0, d]
  const auto div_exact = [](uint64_t x_max, uint32_t d) {
    const uint64_t e = (uint64_t)magic_u32(d) * d - (1ull << 32);
    return x_max < (1ull << 32) && x_max * e < (1ull << 32);
  };
  // the terms that grow with the number of images hold up to some count n_lin: larger batches are launched as ranges of n_lin images
  // (plan_tiling), so that whether the window kernel computes an image depends on per-image dimensions only
  const auto lin_exact = [&](uint64_t nn) {
    return nn * a.ih * a.iw * a.cin * 2 < (1ull << 31) && div_exact(nn * g.hw, (uint32_t)g.hw) && div_exact(nn * g.Sp + 1024, (uint32_t)g.Sp);
  };
  g.n_lin = 0;
  if (div_exact((uint64_t)g.hw, (uint32_t)g.ow) && div_exact((uint64_t)g.Sp, (uint32_t)g.Wp) && lin_exact(1)) {
    // largest count for which lin_exact holds -- NOT capped at n: n_lin must not depend on the batch
    uint64_t lo = 1, hi = (1ull << 31) / ((uint64_t)a.ih * a.iw * a.cin * 2);
    while (lo < hi) {
      const uint64_t mid = (lo + hi + 1) / 2;
      if (lin_exact(mid)) lo = mid; else hi = mid - 1;
    }
    // row_add: a range of n_lin images must end on a group boundary (groups of rows_per_group rows count from row 0 of the tensor)
    const uint64_t rpg = a.row_add ? (uint64_t)a.rows_per_group : 1, step = rpg / std::gcd(rpg, (uint64_t)g.hw);
    g.n_lin = (int32_t)(lo / step * step);  // (< 2^31: lo is)
  }
  g.mul_hw = magic_u32((uint32_t)g.hw);
  g.mul_iw = magic_u32((uint32_t)g.ow);
  g.mul_sp = magic_u32((uint32_t)g.Sp);
  g.mul_wp = magic_u32((uint32_t)g.Wp);
  return true;
}

// Which of the two bitwise-equal 160-column families a launch of M rows x N columns (x `mult` workgroups per tile) takes, from how it
// quantises: see win_candidates.  rows4: tile height of the 4-wave family
inline bool eight_waves_quantise_better(int64_t M, int64_t N, int rows4, int mult) {
  const double tn = (double)((N + 159) / 160) * mult;
  const double t8 = (double)((M + 255) / 256) * tn, t4 = (double)((M + rows4 - 1) / rows4) * tn;
  const double r8 = t8 / 256.0, r4 = t4 / 512.0;
  const double f4 = r4 - (double)(int64_t)r4;
  const double tail4 = f4 > 0.0 ? (f4 <= 0.5 ? 0.55 : 0.55 + 0.9 * (f4 - 0.5)) : 0.0;  // a partly filled round of 4-wave workgroups runs one per CU
  const double cost8 = 0.95 * (double)(int64_t)(r8 + 0.999999) / r8, cost4 = ((double)(int64_t)r4 + tail4) / r4;
  return t8 >= 256.0 && cost8 < cost4;
}

// the kernel's WL (S2: window slots) for output rows [ma, mb] of a linear tile
inline int64_t window_len(const WinCfg& c, const WinProblem& a, const WinGeom& g, int64_t ma, int64_t mb) {
  const auto idx = [&](int64_t m, int64_t& x) {
    const int64_t img = m / g.hw, rem = m % g.hw, y = rem / g.ow;
    x = rem % g.ow;
    if (c.s2) return img * g.Sp + 2 * y * g.Wp + 2 * x;
    return img * g.Sp + ((c.up ? y >> 1 : y) + 1) * g.Wp + (c.up ? x >> 1 : x) + 1;
  };
  int64_t xa, xb;
  const int64_t pa = idx(ma, xa), pb = idx(mb, xb);
  if (c.s2) return ((pb - pa + 2 * g.Wp + 3 + 1) >> 1) * 2;
  const int64_t q0 = (c.up ? pa - (xa >> 1) : pa) - (g.Wp + 1);
  return (c.up ? pb - (xb >> 1) + a.iw - 1 : pb) - q0 + g.Wp + 2;
}
// every linear tile's window <= WCAP; tpi > 0: tiles per image (every image has the same windows), else tiles over `rows` consecutive rows
inline bool fits(const WinCfg& c, const WinProblem& a, const WinGeom& g, int64_t rows, int tpi) {
  const int64_t tiles = tpi > 0 ? (int64_t)tpi : (rows + c.bm - 1) / c.bm;
  const int64_t lim = tpi > 0 ? g.hw : rows;
  for (int64_t t = 0; t < tiles; ++t) {
    const int64_t ma = t * c.bm, mb = ma + c.bm < lim ? ma + c.bm : lim;
    if (window_len(c, a, g, ma, mb - 1) > c.wcap) return false;
  }
  return true;
}

// how one launch of the window kernel tiles its images
struct WinTiling {
  int32_t n;        // images of the launch
  int32_t tpi;      // 0: M-tiles are consecutive BM-pixel ranges of the whole launch; > 0: tiles per image (a tile never leaves its image)
  int32_t tiles_m;
};

constexpr int kMaxWinCandidates = 4;

// The window kernel's part of a plan.  Candidates are tried in order; the first whose window fits one image's tiles wins.  The winner
// launches the batch as n_full ranges of `full.n` images and, if tail.n > 0, one range of tail.n images (2-D tiles: one range, the batch).
struct WinPlan {
  int n_cand = 0;                    // 0: the window kernel does not apply to this conv
  WinCfg cand[kMaxWinCandidates]{};
  int win = -1;                      // index of the winning candidate, -1: every candidate declined
  WinProblem problem{};              // the kernel's view of the conv (phase modes: the source image)
  WinGeom geom{};
  bool linear = false;               // the winner's tiles: consecutive pixels (true) or 16-column 2-D tiles
  int32_t n_full = 0;
  WinTiling full{}, tail{};
  int n_ranges() const { return n_full + (tail.n > 0 ? 1 : 0); }
  const WinTiling& range(int r) const { return r < n_full ? full : tail; }
  void add(const WinCfg& c) { cand[n_cand++] = c; }
};

// Tiling of candidate c, false = it declines.  Whether the linear tiles apply is decided from ONE image: the widest window of a tile of
// consecutive pixels of one image must fit the instantiation's capacity.  (Tiles over consecutive pixels of several images, which may
// straddle an image border, are never narrower than those of image 0 alone, so they cannot widen what applies.)  The output rows are the
// same bits however they are tiled.
inline bool plan_tiling(const WinCfg& c, WinPlan& w) {
  const WinProblem& a = w.problem;
  const WinGeom& g = w.geom;
  if (c.tw > 0) {
    // 2-D tiles: whole tiles only, and (statistics) whole 64-pixel blocks per image
    const int th = c.bm / 16;
    if (a.ow % 16 != 0 || a.oh % th != 0 || g.hw % 64 != 0) return false;
    const int32_t tpi = (a.oh / th) * (a.ow / 16);
    w.linear = false;
    w.n_full = 1;
    w.full = WinTiling{a.n, tpi, (int32_t)((int64_t)a.n * tpi)};
    w.tail = WinTiling{};
    return true;
  }
  if (g.n_lin <= 0 || g.Wp + 1 > c.wcap) return false;
  const int tpi = (g.hw + c.bm - 1) / c.bm;
  if (!fits(c, a, g, g.hw, tpi)) return false;  // the next candidate (2-D tiles, the other family), then the per-tap gather
  // Launches of at most n_lin images (the 31-bit offsets and multiply-high divisions of the linear tiles hold over that range; n_lin
  // comes from per-image dimensions): outputs, residual, row_add and statistics move by whole images.  n_lin keeps a range's first row
  // on a row_add group boundary, and the statistics need hw % 64 == 0, so a range starts on a 64-row block.
  const auto tiling = [&](int32_t nc) {
    // consecutive pixels of the whole range where that fits (a tile may then straddle images: fewer, fuller tiles), else one image's
    // (the scan is bounded: a window of BM pixels + two rows cannot fit once a row exceeds the capacity)
    const int64_t rows = (int64_t)nc * g.hw;
    if (rows / c.bm <= 65536 && fits(c, a, g, rows, 0)) return WinTiling{nc, 0, (int32_t)((rows + c.bm - 1) / c.bm)};
    return WinTiling{nc, tpi, (int32_t)((int64_t)nc * tpi)};
  };
  w.linear = true;
  w.n_full = a.n / g.n_lin;
  w.full = w.n_full > 0 ? tiling(g.n_lin) : WinTiling{};
  w.tail = a.n % g.n_lin ? tiling(a.n % g.n_lin) : WinTiling{};
  return true;
}

// The ordered candidates for a 3x3 conv (stride 1 / pad 1; e4m3: also stride 2 with bottom / right padding), none where the window kernel
// does not apply.  `a` is the launch as gemm.hip's per-tap gather would get it.
inline void win_candidates(const WinProblem& a, int knob, bool fp8, WinPlan& w) {
  w = WinPlan{};
  w.problem = a;
  if (knob == 0) return;
  // e4m3 stride 2 with bottom / right padding only (the VAE encoder's Downsample2D convs in its fp8 mode); the UNet's stride-2 convs (pad 1)
  // and every f16 stride-2 conv keep the per-tap gather
  const bool s2 = fp8 && a.stride == 2 && a.pad_lo == 0 && !a.upsample;
  if (!s2 && (a.stride != 1 || a.pad_lo != 1)) return;
  if (a.a2 || a.sk_ws) return;
  const int up = a.upsample ? 2 : 1;
  if (!s2 && (a.oh != up * a.ih || a.ow != up * a.iw)) return;  // (S2: oh = (ih - 2) / 2 + 1, checked by validate())
  if (a.iw < 2 || a.ih < 2) return;
  const bool narrow = a.N <= 32 && a.N % 4 == 0;  // the UNet's head (4 channels), the VAE's conv_out
  if (a.cin % 64 != 0 || (a.N % 160 != 0 && a.N % 128 != 0 && !narrow) || a.K != 9LL * a.cin) return;
  if (!win_geometry(a, s2, w.geom)) return;
  const bool stats = a.ch_stats;
  if (fp8) {
    // e4m3 operands (the C >= 640 levels in fp8 mode): 128-column tiles only (with 160 columns the 8-register operand tuples of the scaled
    // MFMA no longer fit beside 100 accumulators: 2 KB of scratch; gemm.hip's e4m3 kernels found the same); cin counts 2-byte units
    if (a.N % 128 != 0 || !a.w_exp) return;
    const bool eight = knob == 2;  // two 4-wave workgroups per CU are faster on every e4m3 shape of a step (profiles/r04_kconvwin_fp8.log)
    if (s2) {
      // The VAE encoder's three Downsample2D convs (576 -> 288, 288 -> 144, 144 -> 72 px): the window of a stride-2 tile has about four times
      // its output pixels, so one 4-wave workgroup per CU on 128-row tiles (no 8-wave variant).  Linear tiles where one image's windows fit
      // 864 slots (output rows up to 72 px: a 128-pixel tile spans at most three of them, 846 slots at 72 px), else 2-D tiles of 16 x 8 output
      // pixels (a 17 x 33 source window: 561 slots; 144 and 288 px output rows).
      // Both are decided from one image's dimensions.  No e4m3 output epilogue here (the encoder's downsample output is the fp32 stream).
      // Measured at 7 frames per pass, the family is SLOWER than the e4m3 per-tap gather on all three shapes (255 / 181 / 157 us against
      // 184 / 133 / 110 us: one 4-wave workgroup per CU does not hide the barriers; profiles/r05_kvae_fp8_encode.log), so it runs only when
      // the conv_win knob asks for it (1 or 2); by default these convs keep the gather, as the decoder's families follow the faster kernel.
      if (knob != 1 && knob != 2) return;
      if (a.out_f8) return;
      w.add(win4(128, 128, 864, true).e4m3().stride2());
      w.add(win4(128, 128, 568, true).e4m3().stride2().tiles2d());
      return;
    }
    // The VAE decoder's fp8 mode (128 / 256 / 512 channels, 72 .. 576 px rows) follows the f16 128-column family: linear tiles where the
    // window fits, else 2-D tiles of 16 output columns.  Fused nearest-2x upsample and the e4m3 output epilogue (out_f8: the resnet that
    // feeds an upsample conv writes its A operand) are instantiations of their own; the plain family keeps its linear chain unchanged.
    if (a.upsample) {
      w.add(eight ? win8(128, 416, true).e4m3().upsampled() : win4(128, 128, 288, true).e4m3().upsampled());
      w.add(eight ? win8(128, 104, true).e4m3().upsampled().tiles2d() : win4(128, 128, 64, true).e4m3().upsampled().tiles2d());
    } else if (a.out_f8) {
      w.add(eight ? win8(128, 416, true).e4m3().out8() : win4(128, 128, 288, true).e4m3().out8());
      w.add(eight ? win8(128, 328, true).e4m3().out8().tiles2d() : win4(128, 128, 184, true).e4m3().out8().tiles2d());
    } else {
      w.add(eight ? win8(128, 416, true).e4m3() : win4(128, 128, 288, true).e4m3());
      w.add(eight ? win4(128, 128, 288, true).e4m3() : win8(128, 416, true).e4m3());
      w.add(eight ? win8(128, 328, true).e4m3().tiles2d() : win4(128, 128, 184, true).e4m3().tiles2d());
    }
    return;
  }
  if (narrow) {
    // a conv with a handful of output channels is bound by reading its input: the per-tap gather reads it nine times (head conv of a step:
    // 346 us), the window once.  32-column tile (one MFMA block per wave column; the upper wave column idles when N <= 16)
    if (stats || a.upsample) return;
    w.add(win4(160, 32, 320, false));
    w.add(win4(128, 32, 184, false).tiles2d());
    return;
  }
  if (a.N % 160 != 0) {
    // 128-column family (the VAE's 128 / 256 / 512 channels): linear tiles where the window fits (72 px rows), else 2-D tiles of 16 output
    // columns (144 .. 576 px rows).  Two 4-wave workgroups per CU on 128-row tiles: 2 - 11 % faster than the 8-wave 256-row tile on every
    // decoder shape (profiles/r04_kconvwin_vae.log), which stays behind knob conv_win = 2.
    const bool eight = knob == 2;
    if (a.upsample) {
      w.add(eight ? win8(128, 416, true).upsampled() : win4(128, 128, 288, true).upsampled());
      w.add(eight ? win8(128, 104, true).upsampled().tiles2d() : win4(128, 128, 64, true).upsampled().tiles2d());
    } else {
      w.add(eight ? win8(128, 416, true) : win4(128, 128, 288, true));
      w.add(eight ? win8(128, 328, true).tiles2d() : win4(128, 128, 184, true).tiles2d());
    }
    return;
  }
  if (a.upsample) {
    // fused nearest-2x upsample (the three Upsample convs of a step): the window over the SOURCE image is small (a quarter of the pixels),
    // the 8-wave 256-row tile always fits; the 4-wave family serves launches too small to fill the CUs with 256-row tiles
    const double t8 = (double)((a.M + 255) / 256) * (double)((a.N + 159) / 160);
    const bool eight = knob == 2 || (knob != 1 && t8 >= 256.0);
    const WinCfg c4 = win4(128, 160, 288, true).upsampled(), c8 = win8(160, 416, true).upsampled();
    w.add(eight ? c8 : c4);
    w.add(eight ? c4 : c8);
    return;
  }
  // Two instantiation families, bitwise equal to each other (same reduction order): two 4-wave workgroups per CU on 160-row tiles
  // (128 with statistics) or one 8-wave workgroup on a 256-row tile with the window double-buffered.  The 8-wave tile moves a third
  // fewer LDS-DMA bytes per FLOP and is ~5 % faster where its tile count fills whole rounds of the 256 CUs; the choice is made from
  // how the launch quantises (measured: 72x72 and 18x18 at batch 42 prefer 8 waves, 36x36 prefers 4: tools/kconvwin.py).  Which of
  // the two RUNS may depend on the batch.  Whether the window kernel runs at all depends on per-sample dimensions only: a family applies
  // when one image's tiles fit its window (plan_tiling), statistics need hw % 64 == 0 at every batch size, and a batch too large for the
  // 32-bit index arithmetic of the linear tiles is launched as ranges of whole images (n_lin) instead of falling back to the gather.
  const WinCfg c4 = stats ? win4(128, 160, 288, true) : win4(160, 160, 320, false), c8 = win8(160, 416, true);
  const bool eight = knob == 1 || knob == 2 ? knob == 2 : eight_waves_quantise_better(a.M, a.N, stats ? 128 : 160, 1);
  w.add(eight ? c8 : c4);
  w.add(eight ? c4 : c8);  // the other family may still fit (window capacity is per family)
}

// seva_gemm_desc.upsample = 2 / 4: the nearest-2x upsample + 3x3 conv as four 2x2 phase convs on the source image (conv_win.hip: PH).
// `a0` holds the conv as the caller states it (oh = 2 ih, ow = 2 iw, K = 4 cin, w = [4][N][4 cin]); validate() has refused every epilogue
// but bias + out_f32 (4: + ch_stats).  No candidates = the window kernel does not apply, an ERROR for the caller: no other kernel reads
// this weight layout.
inline void win_phase_candidates(const WinProblem& a0, int knob, WinPlan& w) {
  w = WinPlan{};
  w.problem = a0;
  if (knob == 0) return;
  if (a0.stride != 1 || a0.pad_lo != 1 || a0.oh != 2 * a0.ih || a0.ow != 2 * a0.iw || a0.iw < 2 || a0.ih < 2) return;
  const bool vae = a0.upsample == 4;  // the 128-column family (2-D tiles, statistics); 2: the 160-column one
  if (a0.cin % 64 != 0 || a0.N % (vae ? 128 : 160) != 0 || a0.K != 4LL * a0.cin) return;
  WinProblem& a = w.problem;  // the kernel's view: a plain conv over the SOURCE image, one launch row per source pixel
  a.oh = a0.ih;
  a.ow = a0.iw;
  a.M = (int64_t)a0.n * a0.ih * a0.iw;
  if (!win_geometry(a, false, w.geom)) return;
  if (vae) {
    // As the plain 128-column family: two 4-wave workgroups per CU on 128-row tiles, linear where the window fits (72 px source rows), else
    // 2-D; the 8-wave 256-row tiles behind knob 2.  No other kernel reads these weights, so where the 8-wave tiles do not apply (a 2-D
    // tile of 16 source rows on an image of 8) knob 2 still takes the 4-wave ones: same reduction order, same bits.
    if (knob == 2) {
      w.add(win8(128, 416, true).phases());
      w.add(win8(128, 328, true).phases().tiles2d());
    }
    w.add(win4(128, 128, 288, true).phases());
    w.add(win4(128, 128, 184, true).phases().tiles2d());
    return;
  }
  // the plain conv's two families, bitwise equal (same reduction order), chosen by the same quantisation rule with four workgroups per tile
  const WinCfg c4 = win4(160, 160, 320, false).phases(), c8 = win8(160, 416, false).phases();
  const bool eight = knob == 1 || knob == 2 ? knob == 2 : eight_waves_quantise_better(a.M, a.N, 160, 4);
  w.add(eight ? c8 : c4);
  w.add(eight ? c4 : c8);
}

// first candidate that fits wins
inline void pick_window(WinPlan& w) {
  w.geom.tiles_n = 0;
  for (int i = 0; i < w.n_cand && w.win < 0; ++i)
    if (plan_tiling(w.cand[i], w)) {
      w.win = i;
      w.geom.tiles_n = (int32_t)((w.problem.N + w.cand[i].bn - 1) / w.cand[i].bn);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------------------------------------------------------------

enum Kernel { GEMM_KERNEL = 0, WINDOW_KERNEL = 1 };
// a conv that only the window kernel runs, declined by it: an error, never a fall-back to the gather (messages: gemm.hip)
enum Declined { DECLINED_NONE = 0, DECLINED_PHASES, DECLINED_FP8_STRIDE2, DECLINED_FP8_WINDOW_ONLY };

struct Plan {
  Kernel kernel = GEMM_KERNEL;
  Declined declined = DECLINED_NONE;
  // gemm_kernel (kernel == GEMM_KERNEL)
  GemmCfg gemm{};
  int32_t tiles_m = 0, tiles_n = 0;
  int32_t n_chunks = 0;   // each workgroup walks tiles_n / n_chunks consecutive N-tiles of one M-tile
  int64_t grid = 0;       // workgroups (split-K: two per tile and chunk)
  int32_t dbg = 0, stagger = 0;  // GemmArgs::dbg / stagger of the ablation twin
  // split-K = 2 (gemm.splitk): the caller's workspace must hold sk_tiles tiles of 128 x sk_bn (checked by gemm.hip, which sees its size)
  int64_t sk_tiles = 0;
  int32_t sk_bn = 0;
  // conv_win_kernel: the candidates tried (also when every one declined and the gather runs) and the winner's tiling
  WinPlan window;
};

// N-chunk schedule of gemm_kernel (tiles_m, tiles_n, n_chunks, grid) for the chosen tile shape
inline void plan_chunks(Plan& p, int64_t M, int64_t N, const SevaKnobs& k) {
  const GemmCfg& c = p.gemm;
  p.grid = (M + c.bm - 1) / c.bm;
  if (p.grid > 0x7fffffff) return;  // more M-tiles than a grid has workgroups: the launcher reports the bad grid
  p.tiles_m = (int)p.grid;
  p.tiles_n = (int)((N + c.bn - 1) / c.bn);
  // Schedule: an M-tile's N-tiles are split over `chunks` sibling workgroups that are adjacent in the
  // XCD-remapped order, i.e. co-resident on one XCD: they stream the same A row-panel through that
  // XCD's L2 at the same time.  One workgroup walking ALL N-tiles (the former default for big M)
  // re-reads an 80..320 KB panel per N-tile while 512 such panels (40..160 MB) compete for 32 MB of
  // L2.  Measured over every shape of a step (tools/ksweep_chunks.py, profiles/r01_ksweep_chunks.log):
  // narrow outputs (<= 5 N-tiles) want one tile per workgroup, wide ones ~4 tiles per workgroup, and
  // the split must be even (2,1,1,1 tiles is 30 % slower than 1,1,1,1,1).
  constexpr int kTargetBlocks = 1024;
  const int base = (kTargetBlocks + p.tiles_m - 1) / p.tiles_m;  // >= two rounds of the chip
  int chunks;
  if (p.tiles_n <= 5) {
    chunks = p.tiles_n;
  } else {
    int per = 0;
    for (int t : {4, 5, 3, 2})
      if (p.tiles_n % t == 0) { per = t; break; }
    chunks = per ? p.tiles_n / per : (p.tiles_n + 3) / 4;
  }
  if (c.astat) chunks = 1;  // the A panel sits in registers: re-loading it per sibling is pure cost (re-swept: c1 best)
  if (chunks < base) {
    chunks = base;
    for (int t = base; t <= 2 * base && t <= p.tiles_n; ++t)  // nearest even split above `base`
      if (p.tiles_n % t == 0) { chunks = t; break; }
  }
  // knob gemm_chunks (SEVA_GEMM_CHUNKS=n, benchmarking) overrides the heuristic
  if (k.gemm_chunks > 0) chunks = k.gemm_chunks;
  if (chunks < 1) chunks = 1;
  if (chunks > p.tiles_n) chunks = p.tiles_n;
  p.n_chunks = chunks;
  p.grid = (int64_t)p.tiles_m * chunks;
  if (c.splitk) p.grid *= 2;  // split-K: producers (upper half of K) in the first half of the grid, consumers in the second
}

// The staged-A schedule of a BM x BN tile: PAIRED (the ASYNC schedule of the 2-byte-only outputs and of GEGLU) and the A-in-registers
// variant on top of it.  (The A-in-registers variant is f16-only: with both k-steps' fragments live for one 128-deep MFMA it spills.)
inline GemmCfg tile(int bm, int bn, int mode, int epi, bool fp8, const seva_gemm_desc& d, const SevaKnobs& k) {
  GemmCfg c{bm, bn, mode, epi, false, false, fp8, false, 4, false, false};
  const bool half_out = d.out_f16 || (fp8 && d.out_f8);  // 2-byte (or e4m3) outputs only: ASYNC schedule
  const bool astat_ok = bm == 128 && !fp8 && astat_allowed(k) && d.K <= 320;
  if (epi == 1) {
    c.paired = true;
    c.astat = astat_ok && half_out && !d.out_f32;
  } else if (mode == 0 && bn >= 128 && d.out_f16 && !d.out_f32 && !d.residual) {
    c.paired = true;
    c.astat = astat_ok;
  }
  return c;
}
// a kernel outside the staged-A schedule choice (160-row tiles, split-K, the split-precision output)
inline GemmCfg fixed_tile(int bm, int bn, int mode, int epi) { return GemmCfg{bm, bn, mode, epi, epi == 1, false, false, false, 4, false, false}; }

inline WinProblem win_problem(const seva_gemm_desc& d, Variant v, bool sk) {
  const int ku = v == FP8 ? 2 : 1;  // e4m3 elements per 2-byte unit of the kernel's K / lda / cin arithmetic
  WinProblem a{};
  a.M = d.M; a.N = d.N; a.K = d.K / ku;
  a.n = d.n; a.ih = d.ih; a.iw = d.iw; a.cin = d.cin / ku; a.oh = d.oh; a.ow = d.ow;
  a.stride = d.stride; a.upsample = d.upsample;
  a.pad_lo = d.pad_br_only ? 0 : 1;
  a.rows_per_group = d.rows_per_group > 0 ? d.rows_per_group : 1;
  a.ch_stats = d.ch_stats != nullptr; a.row_add = d.row_add != nullptr; a.out_f8 = d.out_f8 != nullptr; a.w_exp = d.w_exp != nullptr;
  a.a2 = d.a2 != nullptr; a.sk_ws = sk;
  return a;
}

// upsample = 2: the fused nearest-2x upsample as four 2x2 phase convs on the source image (conv_win.hip: PH); w = [4][N][4 cin]
// upsample = 4: the same on the 128-column family, with GroupNorm statistics (the VAE decoders' upsample convs)
inline bool is_phases(const seva_gemm_desc& d) { return d.mode == 1 && (d.upsample == 2 || d.upsample == 4); }

// `d` has passed gemm.hip's validate() for variant v.
inline Plan plan(const seva_gemm_desc& d, const SevaKnobs& k, Variant v) {
  Plan p;
  const auto gemm = [&](const GemmCfg& c) {
    p.kernel = GEMM_KERNEL;
    p.gemm = c;
    p.dbg = k.gemm_dbg > 0 ? k.gemm_dbg : 0;
    p.stagger = k.gemm_stagger > 0 ? k.gemm_stagger : 0;
    p.gemm.dbgk = has_dbgk(c) && (p.dbg || p.stagger);
    plan_chunks(p, d.M, d.N, k);
    return p;
  };
  const auto window = [&]() {
    pick_window(p.window);
    if (p.window.win >= 0) p.kernel = WINDOW_KERNEL;
    return p.window.win >= 0;
  };
  if (is_phases(d)) {
    win_phase_candidates(win_problem(d, v, false), k.conv_win, p.window);
    if (!window()) p.declined = DECLINED_PHASES;
    return p;
  }
  const bool narrow = d.N <= 32;
  if (v == F16_SPLIT_OUT) {
    // one tile shape per epilogue and width, whatever M: nothing about a row's result depends on the batch
    GemmCfg c = d.epilogue == 1 ? fixed_tile(128, 128, 0, 1) : fixed_tile(128, d.N % 160 == 0 ? 160 : 128, 0, 0);
    c.split16 = true;
    return gemm(c);
  }
  // Small problems (the ds8 level: 27 x 8 tiles of 128 rows on 512 workgroup slots) get 64-row tiles: twice the
  // workgroups, both slots of a CU busy.  SEVA_GEMM_BM=64|128 forces the height (benchmark knob).
  bool half_m = ((d.M + 127) / 128) * ((d.N + 159) / 160) < 320 && d.M > 64;
  if (k.gemm_bm > 0) half_m = k.gemm_bm == 64;
  if (d.ch_stats) half_m = false;  // statistics are emitted per wave-owned 64-row block: 128-row tiles only
  // 128x160 tiles: every channel count of the network (320 .. 10240) is a multiple of 160, so no MFMA
  // column is idle (N = 320: 2 tiles instead of 3 with the last half empty), and a tile needs 10 %
  // fewer LDS-DMA bytes and fragment reads per FLOP than 128x128.  (128x64 tiles, tried earlier, were
  // 5-25 % slower: profiles/r01_kbench_bn64.log.)  SEVA_GEMM_BN=128|160 forces the width (benchmark knob).
  bool wide = d.N % 160 == 0;
  if (k.gemm_bn > 0) wide = k.gemm_bn == 160;
  if (v == FP8) {
    // e4m3 operands: the K >= 640 GEMMs / cin >= 640 convs of the ds2..ds8 levels.  Same tile-shape heuristics.
    // (160-row GEGLU tiles, the f16 default, were measured here too: 255 registers with a small spill, no gain)
    if (d.epilogue == 1) return gemm(tile(half_m ? 64 : 128, 128, 0, 1, true, d, k));
    // 128-row tiles are 128 wide only: 128x160 with both k-steps' fragments live exceeds 256 VGPRs (spills)
    const int bm = half_m ? 64 : 128, bn = half_m && wide ? 160 : 128;
    if (d.mode == 0) return gemm(tile(bm, bn, 0, 0, true, d, k));
    // 3x3 / stride 1 / pad 1 convs and the stride-2 bottom / right-padded ones: the window-staged kernel (conv_win.hip, e4m3 instantiations)
    const bool win_on = fp8_window_allowed(k);
    if (d.a2 == nullptr && win_on) {
      win_candidates(win_problem(d, v, false), k.conv_win, true, p.window);
      if (window()) return p;
    }
    // e4m3 stride 2 + pad_br_only (the VAE encoder's fp8 downsample convs): the per-tap gather by default (measured faster, conv_win.hip);
    // where the conv_win knob asks for the stride-2 window family (1 or 2) and it declines, an error, not a silent fall-back to the gather
    if (win_on && (k.conv_win == 1 || k.conv_win == 2) && d.stride == 2 && d.pad_br_only && d.N % 128 == 0) {
      p.declined = DECLINED_FP8_STRIDE2;
      return p;
    }
    // the per-tap gather below has neither the fused upsample nor the e4m3 output in conv mode: only the window kernel runs those
    if (d.upsample || d.out_f8) {
      p.declined = DECLINED_FP8_WINDOW_ONLY;
      return p;
    }
    return gemm(tile(bm, bn, 1, 0, true, d, k));
  }
  const bool two_src = d.mode == 1 && d.a2 != nullptr;  // MODE 3: instantiated for 128- and 160-row tiles, never split-K
  if (two_src) half_m = false;
  // Split-K = 2 for convolutions over SMALL IMAGES (<= SEVA_SPLITK_MAX_PIXELS output pixels per sample: the ds8 level, 9 x 9) with a long
  // reduction: 128-row tiles, two workgroups per tile, instead of 64-row tiles.  The choice looks at per-sample dimensions
  // only, so a sample's result does not depend on the batch size.
  bool sk = false;
  if (d.splitk_ws && d.mode == 1 && !two_src && !d.upsample && !narrow && (int64_t)d.oh * d.ow <= SEVA_SPLITK_MAX_PIXELS && d.K / BK >= 16 &&
      (d.K / BK) % 2 == 0 && tile_height_free(k)) {
    sk = true;
    p.sk_bn = wide ? SEVA_SPLITK_TILE_N : 128;
    p.sk_tiles = ((d.M + SEVA_SPLITK_TILE_M - 1) / SEVA_SPLITK_TILE_M) * ((d.N + p.sk_bn - 1) / p.sk_bn);
    half_m = false;
  }
  // 3x3 / stride 1 / pad 1 convs whose tile window fits LDS: the input window (+ halo) is staged once per 64-channel slab and the nine
  // taps read it through shifted fragment addresses (conv_win.hip); everything else keeps the per-tap gather below
  if (d.mode == 1 && !two_src && tile_shape_free(k)) {
    win_candidates(win_problem(d, v, sk), k.conv_win, false, p.window);
    if (window()) return p;
  }
  if (d.epilogue == 1) {
    // GEGLU tiles are 128 wide (the epilogue pairs 64-row value / gate groups), so the cheaper operand stream comes from the
    // other side: 160 x 128 tiles -- 10 % fewer LDS-DMA bytes per FLOP, 40 instead of 32 MFMAs per wave and barrier, 215
    // registers, still two workgroups per CU.  Bitwise the same outputs; ds2 / ds4 -6 %, the 9x9 level -15 % against its 64-row
    // tiles (tools/kgeglu_bm.py).  K <= 320 keeps the A-in-registers kernel (a 128-row design).
    const bool tall = k.gemm_bm == 160 || (tile_height_free(k) && d.K > 320 && d.M >= 1024);
    if (tall) return gemm(fixed_tile(160, 128, 0, 1));
    return gemm(tile(half_m ? 64 : 128, 128, 0, 1, false, d, k));
  }
  // 160 x 160 tiles for the fp32-output kernels (not the f16-only ASYNC ones: their bias slots would not fit): 0.0125 operand bytes
  // per FLOP instead of 0.0141, 50 instead of 40 MFMAs per wave and barrier; two workgroups take EXACTLY the CU's 160 KiB of LDS
  // and all 256 registers (no spill in GEMM mode, 7 dwords in conv mode).  Bitwise the same outputs; -3 ... -10 % on every shape
  // measured, also where 160-row tiles quantise worse (tools/ktile160.py).  Launches that emit GroupNorm statistics keep 128
  // rows (a wave must own a 64-row block), as do the small ones (64-row tiles / split-K) and the fused-upsample conv.
  const int mode = two_src ? 3 : d.mode == 0 ? 0 : d.upsample ? 2 : 1;  // (2: the three Upsample convs of a step, general gather)
  const bool f16_only = d.mode == 0 && d.out_f16 && !d.out_f32 && !d.residual;
  const bool big = k.gemm_bm == 160 || (tile_shape_free(k) && !half_m && d.M >= 2048);
  if (big && wide && !narrow && !d.ch_stats && !d.upsample && !sk && !f16_only) return gemm(fixed_tile(160, 160, mode, 0));
  const int bn = wide ? 160 : 128;
  if (two_src) return gemm(tile(128, bn, 3, 0, false, d, k));
  if (narrow) return gemm(tile(128, 32, mode, 0, false, d, k));
  if (sk) {
    GemmCfg c = fixed_tile(128, bn, 1, 0);
    c.splitk = true;
    return gemm(c);
  }
  return gemm(tile(half_m ? 64 : 128, bn, mode, 0, false, d, k));
}

}  // namespace seva_plan
