// LPIPS v0.1 (Zhang et al. 2018), VGG-16 backbone: what the 13 convolutions (seva_gemm_f16, conv mode) leave to do.  The arithmetic
// contract of the three operators is in include/seva_hip.h.  Like metrics.hip the file is built with -ffp-contract=off and spells each
// fp32 operation as an __f*_rn intrinsic: every operation is rounded on its own, the expressions of the two frames are the same
// operations in the same order (a frame against itself is exactly 0, d(a, b) == d(b, a) bit for bit), and the contract can be restated
// in plain torch (tests/fake_lpips_ops.py).
//
//   lpips_prepare_kernel     uint8 NHWC / fp32 NCHW frames -> the scaling layer's output as the 64-channel padded f16 NHWC operand of
//                            the first conv; eight lanes per pixel, one 16-byte store each
//   lpips_relu_pool_kernel   ReLU of a conv's f16 output (in place or not) and, where asked, the 2 x 2 / stride-2 max-pool of the
//                            ReLU'd values; one lane per 2 x 2 block and 8 channels, 16-byte accesses
//   lpips_layer_kernel       per pixel: unit-normalise both feature vectors over the channels, d = sum_c w[c] (na_c - nb_c)^2.  C / 8
//                            lanes hold a pixel (8 channels = one 16-byte load per operand and lane); two xor-butterflies give every lane
//                            the two norms, a third gives d.  A workgroup covers 256 consecutive pixels of one frame pair; the
//                            pixels' d are widened to fp64, summed per lane in pixel order and then by the fixed tree (block_tree,
//                            frame_common.h) into the slab
//                            [n][chunks]
//   lpips_sum_kernel         one workgroup per pair folds its slab row in a fixed order (slab_fold, frame_common.h)
// No atomics: the result of a pair depends on that pair alone and repeats bit for bit.
#include <math.h>

#include "frame_common.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_PIXELS = 256;  // pixels of one frame pair per workgroup of the layer kernel
constexpr int LP_CPAD = 64;     // channels of the prepared operand

struct LpipsScaling {
  float shift[3], scale[3];
};

template <int KIND>
__global__ __launch_bounds__(LP_THREADS) void lpips_prepare_kernel(const void* __restrict__ src, const int64_t pitch_n, half_t* __restrict__ out,
                                                                   const int64_t pixels, const int64_t hw, const LpipsScaling sc) {
  const int64_t gid = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
  const int64_t pix = gid >> 3;
  const int sub = (int)(gid & 7);
  if (pix >= pixels) return;
  half8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (sub == 0) {
    const int64_t img = pix / hw, p = pix - img * hw;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t u;
      if (KIND == FRAME_U8)
        u = ((const uint8_t*)src)[img * pitch_n + p * 3 + c];
      else
        u = frame_u8(((const float*)src)[img * pitch_n + (int64_t)c * hw + p]);
      float x = __fsub_rn(__fdiv_rn((float)u, 127.5f), 1.0f);
      x = __fdiv_rn(__fsub_rn(x, sc.shift[c]), sc.scale[c]);
      v[c] = (half_t)x;  // one round-to-nearest-even
    }
  }
  *(half8_t*)(out + pix * LP_CPAD + sub * 8) = v;
}

// max(v, 0) with torch's NaN rule: a NaN stays a NaN
__device__ __forceinline__ half8_t relu8(half8_t v) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = v[i] <= (half_t)0 ? (half_t)0 : v[i];
  return v;
}
// running maximum with torch's NaN rule: a NaN wins
__device__ __forceinline__ half8_t max8(half8_t m, half8_t v) {
#pragma unroll
  for (int i = 0; i < 8; ++i) m[i] = (v[i] > m[i] || v[i] != v[i]) ? v[i] : m[i];
  return m;
}

// one lane: 8 channels of the 2 x 2 block (by, bx) of one image.  x and relu_out may be the same tensor (a lane reads the elements it
// writes, nothing else)
template <bool POOL>
__global__ __launch_bounds__(LP_THREADS) void lpips_relu_pool_kernel(const half_t* x, half_t* relu_out, half_t* __restrict__ pool_out,
                                                                     const int64_t total, const int h, const int w, const int c) {
  const int64_t gid = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
  if (gid >= total) return;
  const int cv = c >> 3, bh = (h + 1) >> 1, bw = (w + 1) >> 1;
  const int v = (int)(gid % cv);
  int64_t r = gid / cv;
  const int bx = (int)(r % bw);
  r /= bw;
  const int by = (int)(r % bh);
  const int64_t img = r / bh;
  half8_t q[2][2];
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int y = 2 * by + dy, xx = 2 * bx + dx;
      if (y < h && xx < w) {
        const int64_t off = ((img * h + y) * w + xx) * c + v * 8;
        q[dy][dx] = relu8(*(const half8_t*)(x + off));
        *(half8_t*)(relu_out + off) = q[dy][dx];
      }
    }
  if (POOL && 2 * by + 1 < h && 2 * bx + 1 < w) {  // floor: an odd last row / column has no block
    const half8_t m = max8(max8(max8(q[0][0], q[0][1]), q[1][0]), q[1][1]);
    *(half8_t*)(pool_out + ((img * (h >> 1) + by) * (w >> 1) + bx) * c + v * 8) = m;
  }
}

// correctly rounded (hipcc's default for sqrtf in HIP code); __fsqrt_rn is the 1-ulp native instruction in this toolchain's headers
__device__ __forceinline__ float sqrt_rn(float v) { return __builtin_sqrtf(v); }

// sum over the L lanes of a pixel, the same value in every lane: s = s + s[lane ^ o] for o = L/2, L/4, .. 1
template <int L>
__device__ __forceinline__ float pixel_sum(float s) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) s = __fadd_rn(s, first_read(__shfl_xor(s, o, 64)));
  return s;
}

template <int L>  // lanes per pixel: C = 8 L
__global__ __launch_bounds__(LP_THREADS) void lpips_layer_kernel(const half_t* __restrict__ fa, const half_t* __restrict__ fb,
                                                                 const int64_t pitch_a, const int64_t pitch_b, const float* __restrict__ w,
                                                                 const int64_t hw, const int chunks, double* __restrict__ part) {
  __shared__ double red[LP_THREADS];
  constexpr int G = LP_THREADS / L;  // pixels in flight per workgroup
  constexpr int C = 8 * L;
  const int t = threadIdx.x, g = t / L, j = t - g * L;
  const int64_t img = blockIdx.x / chunks;
  const int64_t p0 = (int64_t)(blockIdx.x - img * chunks) * LP_PIXELS;
  const half_t* pa = fa + img * pitch_a + j * 8;
  const half_t* pb = fb + img * pitch_b + j * 8;
  float wv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) wv[i] = first_read(w[j * 8 + i]);

  double acc = 0.0;
#pragma unroll 4
  for (int k = 0; k < LP_PIXELS / G; ++k) {
    const int64_t p = p0 + (int64_t)k * G + g;
    const bool ok = p < hw;  // (a pixel beyond the frame computes on zeros and is not added)
    half8_t va = {0, 0, 0, 0, 0, 0, 0, 0}, vb = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) {
      va = *(const half8_t*)(pa + p * C);
      vb = *(const half8_t*)(pb + p * C);
    }
    float a[8], b[8];
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      a[i] = first_read((float)va[i]);
      b[i] = first_read((float)vb[i]);
      sa = __fadd_rn(sa, __fmul_rn(a[i], a[i]));
      sb = __fadd_rn(sb, __fmul_rn(b[i], b[i]));
    }
    const float ra = __fdiv_rn(1.0f, __fadd_rn(sqrt_rn(pixel_sum<L>(sa)), 1e-10f));  // one division per vector, not one per channel
    const float rb = __fdiv_rn(1.0f, __fadd_rn(sqrt_rn(pixel_sum<L>(sb)), 1e-10f));
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float df = __fsub_rn(__fmul_rn(a[i], ra), __fmul_rn(b[i], rb));
      d = __fadd_rn(d, __fmul_rn(wv[i], __fmul_rn(df, df)));
    }
    d = pixel_sum<L>(d);
    if (ok && j == 0) acc += (double)d;
  }
  const double s = block_tree<LP_THREADS>(acc, red, [](double a, double b) { return a + b; });
  if (t == 0) part[blockIdx.x] = s;
}

// one workgroup per pair folds its row of the slab
__global__ __launch_bounds__(LP_THREADS) void lpips_sum_kernel(const double* __restrict__ part, const int chunks, double* __restrict__ out) {
  __shared__ double red[LP_THREADS];
  const int t = threadIdx.x, img = blockIdx.x;
  const double s = slab_fold<LP_THREADS>(0.0, chunks, [&](int i) { return part[(int64_t)img * chunks + i]; }, red,
                                         [](double a, double b) { return a + b; });
  if (t == 0) out[img] = s;
}

inline int64_t layer_chunks(int64_t hw) { return (hw + LP_PIXELS - 1) / LP_PIXELS; }

}  // namespace

extern "C" int seva_lpips_prepare_f16(const void* src, int64_t src_pitch_n, int32_t kind, void* out_f16, int32_t n, int32_t H, int32_t W,
                                      seva_stream_t stream) {
  SEVA_REQUIRE(src && out_f16, "lpips_prepare: null src or out_f16");
  SEVA_REQUIRE(n > 0 && H > 0 && W > 0, "lpips_prepare: bad sizes n=%d H=%d W=%d", n, H, W);
  if (int rc = frame_checks("lpips_prepare", kind, H, W, src, src_pitch_n)) return rc;
  const int64_t hw = (int64_t)H * W;
  SEVA_REQUIRE((((uintptr_t)out_f16) & 15) == 0, "lpips_prepare: out_f16 must be 16-byte aligned");
  const int64_t pixels = (int64_t)n * hw;
  const int64_t blocks = (pixels * 8 + LP_THREADS - 1) / LP_THREADS;
  SEVA_REQUIRE(grid_fits(blocks), "lpips_prepare: n*H*W = %lld exceeds the grid", (long long)pixels);
  const LpipsScaling sc = {{-.030f, -.088f, -.188f}, {.458f, .448f, .450f}};
  hipStream_t s = (hipStream_t)stream;
  SevaProfScope prof(4, (double)pixels * (LP_CPAD * 2.0 + (kind == FRAME_U8 ? 3.0 : 12.0)), s);
  if (kind == FRAME_U8)
    hipLaunchKernelGGL(lpips_prepare_kernel<FRAME_U8>, dim3((unsigned)blocks), dim3(LP_THREADS), 0, s, src, src_pitch_n, (half_t*)out_f16,
                       pixels, hw, sc);
  else
    hipLaunchKernelGGL(lpips_prepare_kernel<FRAME_F32>, dim3((unsigned)blocks), dim3(LP_THREADS), 0, s, src, src_pitch_n, (half_t*)out_f16,
                       pixels, hw, sc);
  return seva_check_launch("lpips_prepare_kernel");
}

extern "C" int seva_lpips_relu_pool_f16(const void* x, void* relu_out, void* pool_out, int32_t n, int32_t h, int32_t w, int32_t c,
                                        seva_stream_t stream) {
  SEVA_REQUIRE(x && relu_out, "lpips_relu_pool: null x or relu_out");
  SEVA_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && c % 64 == 0, "lpips_relu_pool: bad sizes n=%d h=%d w=%d c=%d (c %% 64 == 0)", n, h, w, c);
  SEVA_REQUIRE(!pool_out || (h >= 2 && w >= 2), "lpips_relu_pool: the 2 x 2 pool needs h, w >= 2, got %d x %d", h, w);
  SEVA_REQUIRE(((((uintptr_t)x) | ((uintptr_t)relu_out) | ((uintptr_t)pool_out)) & 15) == 0, "lpips_relu_pool: tensors must be 16-byte aligned");
  SEVA_REQUIRE(pool_out != x && pool_out != relu_out, "lpips_relu_pool: pool_out must not be x or relu_out");
  const int64_t total = (int64_t)n * ((h + 1) / 2) * ((w + 1) / 2) * (c / 8);
  const int64_t blocks = (total + LP_THREADS - 1) / LP_THREADS;
  SEVA_REQUIRE(grid_fits(blocks), "lpips_relu_pool: %lld lanes exceed the grid", (long long)total);
  hipStream_t s = (hipStream_t)stream;
  const double elems = (double)n * h * w * c;
  SevaProfScope prof(4, elems * 4.0 + (pool_out ? (double)n * (h / 2) * (w / 2) * c * 2.0 : 0.0), s);
  if (pool_out)
    hipLaunchKernelGGL(lpips_relu_pool_kernel<true>, dim3((unsigned)blocks), dim3(LP_THREADS), 0, s, (const half_t*)x, (half_t*)relu_out,
                       (half_t*)pool_out, total, h, w, c);
  else
    hipLaunchKernelGGL(lpips_relu_pool_kernel<false>, dim3((unsigned)blocks), dim3(LP_THREADS), 0, s, (const half_t*)x, (half_t*)relu_out,
                       (half_t*)nullptr, total, h, w, c);
  return seva_check_launch("lpips_relu_pool_kernel");
}

extern "C" int seva_lpips_layer_size(int32_t n, int64_t hw, int64_t* workspace_bytes) {
  SEVA_REQUIRE(n > 0 && hw > 0 && workspace_bytes, "lpips_layer_size: bad arguments n=%d hw=%lld", n, (long long)hw);
  *workspace_bytes = (int64_t)n * layer_chunks(hw) * 8;  // one fp64 partial per 256 pixels of every pair
  return SEVA_OK;
}

extern "C" int seva_lpips_layer(const seva_lpips_layer_desc* d, seva_stream_t stream) {
  SEVA_REQUIRE(d && d->fa && d->fb && d->w && d->out && d->workspace, "lpips_layer: null descriptor, fa, fb, w, out or workspace");
  SEVA_REQUIRE(d->n > 0 && d->hw > 0, "lpips_layer: bad sizes n=%d hw=%lld", d->n, (long long)d->hw);
  SEVA_REQUIRE(d->C == 64 || d->C == 128 || d->C == 256 || d->C == 512, "lpips_layer: C=%d (64, 128, 256 or 512)", d->C);
  const int64_t elems = d->hw * d->C;
  SEVA_REQUIRE(d->a_pitch_n >= elems && d->b_pitch_n >= elems && d->a_pitch_n % 8 == 0 && d->b_pitch_n % 8 == 0,
               "lpips_layer: frame pitches (%lld, %lld) must be >= hw*C and multiples of 8", (long long)d->a_pitch_n, (long long)d->b_pitch_n);
  SEVA_REQUIRE(((((uintptr_t)d->fa) | ((uintptr_t)d->fb)) & 15) == 0 && (((uintptr_t)d->w) & 3) == 0 && (((uintptr_t)d->out) & 7) == 0,
               "lpips_layer: fa, fb must be 16-byte, w 4-byte, out 8-byte aligned");
  const int64_t chunks = layer_chunks(d->hw);
  const int64_t blocks = (int64_t)d->n * chunks;
  SEVA_REQUIRE(grid_fits(blocks), "lpips_layer: n * chunks = %lld exceeds the grid", (long long)blocks);
  SEVA_REQUIRE(d->workspace_bytes >= blocks * 8 && (((uintptr_t)d->workspace) & 7) == 0,
               "lpips_layer: workspace of %lld bytes (need %lld, 8-byte aligned)", (long long)d->workspace_bytes, (long long)(blocks * 8));
  double* part = (double*)d->workspace;
  hipStream_t s = (hipStream_t)stream;
  SevaProfScope prof(4, (double)d->n * elems * 4.0, s);
#define LPIPS_LAYER(L)                                                                                                          \
  hipLaunchKernelGGL(lpips_layer_kernel<L>, dim3((unsigned)blocks), dim3(LP_THREADS), 0, s, (const half_t*)d->fa, (const half_t*)d->fb, \
                     d->a_pitch_n, d->b_pitch_n, d->w, d->hw, (int)chunks, part)
  switch (d->C) {
    case 64: LPIPS_LAYER(8); break;
    case 128: LPIPS_LAYER(16); break;
    case 256: LPIPS_LAYER(32); break;
    default: LPIPS_LAYER(64); break;
  }
#undef LPIPS_LAYER
  if (int rc = seva_check_launch("lpips_layer_kernel")) return rc;
  hipLaunchKernelGGL(lpips_sum_kernel, dim3((unsigned)d->n), dim3(LP_THREADS), 0, s, part, (int)chunks, d->out);
  return seva_check_launch("lpips_sum_kernel");
}
