// Benchmark / debugging knobs (capi.hip).  Read ONCE from the SEVA_* environment when the library is loaded (no
// getenv on the launch path); tests and tools change them at run time through seva_set_knob().  -1 = unset.
// Plain C++: the dispatch planner (gemm_plan.h) takes the knobs as an argument and compiles without HIP.
#pragma once

struct SevaKnobs {
  int gemm_chunks, gemm_dbg, gemm_stagger, gemm_bm, gemm_bn, gemm_astat;
  int attn_dbg, attn_no_tr, attn_two, attn_split;
  int attn_short2;  // 32 < lq <= 64, lk <= 64: 1 = two waves on one K/V buffer, 0 = attn_kernel<4, 64>; unset: the library's default
  int gn_min_iter;
  int conv_win;  // 0: per-tap gather everywhere; 1: window kernel, two 4-wave workgroups per CU; 2: 8-wave 256-row tile; unset: default
};
extern SevaKnobs g_seva_knobs;
