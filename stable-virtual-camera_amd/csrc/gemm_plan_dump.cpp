// Prints the dispatch plan (gemm_plan.h) of descriptors read from stdin: the planner's consumer outside the library, plain C++17
// (g++ -std=c++17 gemm_plan_dump.cpp), no GPU.  tests/test_gemm_plan_cpu.py drives it.
//
// One descriptor per line, `key=value` tokens separated by blanks; what is not named is 0 / null / knob unset (-1):
//   v=f16|split_out|fp8   mode epi M N K   n ih iw cin oh ow stride up pad_br   rpg K2
//   pointers (1 = set): bias row_add residual out_f32 out_f16 out_f8 w_exp ch_stats splitk_ws a2
//   knobs: gemm_bm gemm_bn gemm_astat gemm_chunks gemm_dbg gemm_stagger conv_win
// The descriptor must be one that gemm.hip's validate() accepts (the planner's precondition).  The line `tables` prints the two
// instantiation tables instead.  One tab-separated output line per input line.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "gemm_plan.h"

using namespace seva_plan;

static void print_gemm_cfg(const GemmCfg& c) {
  printf("\tbm=%d\tbn=%d\tmode=%d\tepi=%d\tdbgk=%d\tpaired=%d\tastat=%d\tfp8=%d\tsplitk=%d\tnw=%d\tsplit16=%d", c.bm, c.bn, c.mode, c.epi, c.dbgk,
         c.paired, c.astat, c.fp8, c.splitk, c.nw, c.split16);
}
static void print_win_cfg(const WinCfg& c) {
  printf("\tbm=%d\tbn=%d\tnw=%d\twcap=%d\tdbw=%d\tstats=%d\tup=%d\ttw=%d\tfp8=%d\to8=%d\ts2=%d\tph=%d", c.bm, c.bn, c.nw, c.wcap, c.dbw, c.stats,
         c.up, c.tw, c.fp8, c.o8, c.s2, c.ph);
}

static int print_tables() {
  for (int i = 0; i < kNumGemmKernels; ++i) {
    printf("table=gemm\trow=%d\tname=%s\thas_dbgk=%d", i, kGemmKernels[i].name, has_dbgk(kGemmKernels[i].cfg));
    print_gemm_cfg(kGemmKernels[i].cfg);
    printf("\n");
  }
  for (int i = 0; i < kNumWinKernels; ++i) {
    printf("table=win\trow=%d\tname=%s", i, kWinKernels[i].name);
    print_win_cfg(kWinKernels[i].cfg);
    printf("\n");
  }
  return 0;
}

int main() {
  static char line[4096];
  void* const set = (void*)(uintptr_t)64;  // never dereferenced: the planner looks at null-ness only
  while (fgets(line, sizeof line, stdin)) {
    if (strncmp(line, "tables", 6) == 0) {
      print_tables();
      continue;
    }
    seva_gemm_desc d;
    memset(&d, 0, sizeof d);
    SevaKnobs k;
    k.gemm_chunks = k.gemm_dbg = k.gemm_stagger = k.gemm_bm = k.gemm_bn = k.gemm_astat = -1;
    k.attn_dbg = k.attn_no_tr = k.attn_two = k.attn_split = k.attn_short2 = k.gn_min_iter = k.conv_win = -1;
    Variant v = F16;
    bool any = false, bad = false;
    for (char* tok = strtok(line, " \t\r\n"); tok; tok = strtok(nullptr, " \t\r\n")) {
      char* eq = strchr(tok, '=');
      if (!eq) { bad = true; break; }
      *eq = 0;
      const std::string key = tok, val = eq + 1;
      const long long x = atoll(val.c_str());
      any = true;
      if (key == "v") v = val == "fp8" ? FP8 : val == "split_out" ? F16_SPLIT_OUT : F16;
      else if (key == "mode") d.mode = (int)x;
      else if (key == "epi") d.epilogue = (int)x;
      else if (key == "M") d.M = x;
      else if (key == "N") d.N = x;
      else if (key == "K") d.K = x;
      else if (key == "n") d.n = (int)x;
      else if (key == "ih") d.ih = (int)x;
      else if (key == "iw") d.iw = (int)x;
      else if (key == "cin") d.cin = (int)x;
      else if (key == "oh") d.oh = (int)x;
      else if (key == "ow") d.ow = (int)x;
      else if (key == "stride") d.stride = (int)x;
      else if (key == "up") d.upsample = (int)x;
      else if (key == "pad_br") d.pad_br_only = (int)x;
      else if (key == "rpg") d.rows_per_group = x;
      else if (key == "K2") d.K2 = x;
      else if (key == "bias") d.bias = x ? (const float*)set : nullptr;
      else if (key == "row_add") d.row_add = x ? (const float*)set : nullptr;
      else if (key == "residual") d.residual = x ? (const float*)set : nullptr;
      else if (key == "out_f32") d.out_f32 = x ? (float*)set : nullptr;
      else if (key == "out_f16") d.out_f16 = x ? set : nullptr;
      else if (key == "out_f8") d.out_f8 = x ? set : nullptr;
      else if (key == "w_exp") d.w_exp = x ? set : nullptr;
      else if (key == "ch_stats") d.ch_stats = x ? (float*)set : nullptr;
      else if (key == "splitk_ws") d.splitk_ws = x ? (float*)set : nullptr;
      else if (key == "a2") d.a2 = x ? set : nullptr;
      else if (key == "gemm_bm") k.gemm_bm = (int)x;
      else if (key == "gemm_bn") k.gemm_bn = (int)x;
      else if (key == "gemm_astat") k.gemm_astat = (int)x;
      else if (key == "gemm_chunks") k.gemm_chunks = (int)x;
      else if (key == "gemm_dbg") k.gemm_dbg = (int)x;
      else if (key == "gemm_stagger") k.gemm_stagger = (int)x;
      else if (key == "conv_win") k.conv_win = (int)x;
      else { bad = true; break; }
    }
    if (!any) continue;
    if (bad) {
      printf("kernel=bad_input\n");
      continue;
    }
    d.a = set;
    d.w = set;
    const Plan p = plan(d, k, v);
    const WinPlan& w = p.window;
    static const char* const declined[] = {"none", "phases", "fp8_stride2", "fp8_window_only"};
    if (p.declined != DECLINED_NONE) {
      printf("kernel=error\tdeclined=%s", declined[p.declined]);
    } else if (p.kernel == GEMM_KERNEL) {
      const int row = find_row(p.gemm);
      printf("kernel=gemm\trow=%d\tname=%s", row, row >= 0 ? kGemmKernels[row].name : "NONE");
      print_gemm_cfg(p.gemm);
      printf("\ttiles_m=%d\ttiles_n=%d\tchunks=%d\tgrid=%lld\tdbg=%d\tstagger=%d\tsk_tiles=%lld\tsk_bn=%d", p.tiles_m, p.tiles_n, p.n_chunks,
             (long long)p.grid, p.dbg, p.stagger, (long long)p.sk_tiles, p.sk_bn);
    } else {
      const WinCfg& c = w.cand[w.win];
      const int row = find_row(c);
      printf("kernel=window\trow=%d\tname=%s", row, row >= 0 ? kWinKernels[row].name : "NONE");
      print_win_cfg(c);
      printf("\tlinear=%d\tn_lin=%d\tranges=%d\tn_full=%d\tfull=%d/%d/%d\ttail=%d/%d/%d\ttiles_n=%d", w.linear, w.geom.n_lin, w.n_ranges(), w.n_full,
             w.full.n, w.full.tpi, w.full.tiles_m, w.tail.n, w.tail.tpi, w.tail.tiles_m, w.geom.tiles_n);
      printf("\tWp=%d\tSp=%d\thw=%d\tow=%d\tmul=%u/%u/%u/%u", w.geom.Wp, w.geom.Sp, w.geom.hw, w.geom.ow, w.geom.mul_hw, w.geom.mul_iw, w.geom.mul_sp,
             w.geom.mul_wp);
    }
    // the window candidates tried, in order (also where every one declined and the gather runs); a name NONE = not in the table
    printf("\twin=%d\tcands=", w.win);
    for (int i = 0; i < w.n_cand; ++i) {
      const int row = find_row(w.cand[i]);
      printf("%s%s", i ? ";" : "", row >= 0 ? kWinKernels[row].name : "NONE");
    }
    printf("\n");
  }
  return 0;
}
