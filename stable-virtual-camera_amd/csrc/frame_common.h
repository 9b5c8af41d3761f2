// What the frame-score and audit kernels share (frames.hip, metrics.hip, lpips.hip, range.hip): the uint8 rule of a saved frame, the
// two frame kinds with their host checks, and the fixed-order workgroup reduction whose order is the repeatability contract.
//
// The fp32 functions here are exact only in a translation unit built with -ffp-contract=off (frames, metrics, lpips: FLAGS_<stem> of
// the Makefile); for the same reason they are spelled with __f*_rn intrinsics, so that no FMA and no reciprocal-multiply can form
// whatever the flags are.  range.hip (integer tests only) takes the reduction and nothing in fp32.
#pragma once

#include "seva_common.h"

// frame operands: seva_metrics_desc.kind, seva_lpips_prepare_f16's kind (the ABI's values)
enum { FRAME_U8 = 0, FRAME_F32 = 1 };  // uint8 NHWC / fp32 NCHW

// (v + 1) / 2 * 255 -> clamp -> truncate; the comparisons are false for a NaN, which therefore gives 0
__device__ __forceinline__ uint32_t frame_u8(float v) {
  float t = __fdiv_rn(__fadd_rn(v, 1.0f), 2.0f);
  t = __fmul_rn(t, 255.0f);
  t = t > 0.0f ? t : 0.0f;
  t = t < 255.0f ? t : 255.0f;
  return (uint32_t)(int)t;
}

// host side: the argument checks of operator `who`'s frame operand(s): kind, image pitch, fp32 alignment (b: a pair's second frame)
inline int frame_checks(const char* who, int kind, int32_t H, int32_t W, const void* a, int64_t a_pitch_n, const void* b = nullptr,
                        int64_t b_pitch_n = 0) {
  SEVA_REQUIRE(kind == FRAME_U8 || kind == FRAME_F32, "%s: kind=%d (0: uint8 NHWC, 1: fp32 NCHW)", who, kind);
  const int64_t elems = 3 * (int64_t)H * W;
  if (b)
    SEVA_REQUIRE(a_pitch_n >= elems && b_pitch_n >= elems, "%s: image pitches (%lld, %lld) < 3*H*W", who, (long long)a_pitch_n,
                 (long long)b_pitch_n);
  else
    SEVA_REQUIRE(a_pitch_n >= elems, "%s: image pitch %lld < 3*H*W", who, (long long)a_pitch_n);
  SEVA_REQUIRE(kind == FRAME_U8 || ((((uintptr_t)a) | ((uintptr_t)b)) & 3) == 0, "%s: fp32 frames must be 4-byte aligned", who);
  return SEVA_OK;
}

inline bool grid_fits(int64_t blocks) { return blocks <= 0x7fffffffLL; }

// Two reductions under the same barriers (a (double, integer) pair, (max, min)): the pair's value and its scratch.  The scratch stays
// two arrays: a (double, u32) pair costs 12 bytes a thread, not a padded 16.
template <class A, class B>
struct Pair { A a; B b; };
template <class A, class B>
struct PairRed {
  A *a; B *b;
  struct Ref {
    A &a; B &b;
    __device__ __forceinline__ operator Pair<A, B>() const { return {a, b}; }
    __device__ __forceinline__ void operator=(Pair<A, B> v) const { a = v.a, b = v.b; }
  };
  __device__ __forceinline__ Ref operator[](int i) const { return {a[i], b[i]}; }
};

// THE fixed-order tree of a THREADS-thread workgroup: red[t] = v; then red[t] op= red[t + s] for s = THREADS / 2 .. 1 where t < s, one
// barrier per level; every thread gets red[0].  tests/fake_lpips_ops.py::_tree and tests/fake_range_ops.py restate this order.
// red: T* (THREADS values of LDS), or a PairRed for T = Pair; op: T x T -> T (sum, max, min); a caller that uses the same `red` again
// puts a barrier in between.
template <int THREADS, class T, class Red, class Op>
__device__ __forceinline__ T block_tree(T v, Red red, Op op) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = op(T(red[t]), T(red[t + s]));
    __syncthreads();
  }
  return red[0];
}

// second stage over a slab of `items` partials: thread t folds items t, t + THREADS, ... in that order (from `init`), then the tree
template <int THREADS, class T, class I, class Load, class Red, class Op>
__device__ __forceinline__ T slab_fold(T init, I items, Load load, Red red, Op op) {
  T v = init;
  for (I i = threadIdx.x; i < items; i += THREADS) v = op(v, T(load(i)));
  return block_tree<THREADS>(v, red, op);
}
