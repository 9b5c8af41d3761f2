// Image-space scores of generated frames against held-out pictures: per-frame sum of squared errors (-> MSE / PSNR) and SSIM
// (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, valid positions) on the uint8 frames a user would save.  The arithmetic
// contract is in include/seva_hip.h.  Like frames.hip the file is built with -ffp-contract=off and spells each fp32 operation as an
// __f*_rn intrinsic: every operation is rounded on its own, the expressions of the two frames are the same operations in the same
// order (ssim(a, a) is exactly 1), and the contract can be restated in plain torch (tests/fake_metric_ops.py).
//
// One 256-thread workgroup per 32 x 32 tile of one image: the 42 x 42 halo of both frames is staged in LDS as bytes (fp32 sources
// go through the uint8 rule on the way in), the tile's squared error is summed from the staged bytes, and per channel a horizontal
// pass writes five LDS planes (x, y, xx, yy, xy) whose vertical pass and SSIM expression stay in registers.  Partials are reduced by
// the fixed-order tree of frame_common.h and written to a slab [n][tiles]; a second kernel (one workgroup per image) folds the slab
// in a fixed order (slab_fold, frame_common.h).
// No atomics: the result of an image depends on that image alone and repeats bit for bit.
#include <math.h>

#include "frame_common.h"

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_TILE = 32;                       // output positions per tile side
constexpr int MT_WIN = 11;                        // Gaussian window
constexpr int MT_HALO = MT_TILE + MT_WIN - 1;     // 42 staged rows / pixels per row
constexpr int MT_ROW_WORDS = 32;                  // staged row pitch: 128 bytes >= 42 * 3
constexpr int MT_ROW_BYTES = 4 * MT_ROW_WORDS;
constexpr int MT_STAGE_WORDS = MT_HALO * MT_ROW_WORDS;

struct MetricsWeights {
  float g[MT_WIN];
};

// Stages rows y0 .. y0+41, bytes 3*x0 .. 3*x0+127 of one frame's row-interleaved RGB into `st`; everything outside the image is 0.
template <int KIND>
__device__ __forceinline__ void stage_frame(uint32_t* st, const void* base, int64_t pitch_n, int img, int H, int W, int y0, int x0) {
  const int t = threadIdx.x;
  const int64_t rowb = (int64_t)W * 3;
  if (KIND == FRAME_U8) {
    const uint8_t* src = (const uint8_t*)base + (int64_t)img * pitch_n;
    const bool aligned = ((((uintptr_t)src) | (uintptr_t)rowb) & 3) == 0;  // 3 * x0 = 96 * tile is a multiple of 4
    for (int i = t; i < MT_STAGE_WORDS; i += MT_THREADS) {
      const int r = i / MT_ROW_WORDS, w = i - r * MT_ROW_WORDS;
      const int y = y0 + r;
      const int64_t off = (int64_t)x0 * 3 + 4 * w;
      uint32_t v = 0;
      if (y < H && off < rowb) {
        const uint8_t* p = src + (int64_t)y * rowb + off;
        if (aligned && off + 4 <= rowb) {
          v = *(const uint32_t*)p;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (off + k < rowb) v |= (uint32_t)p[k] << (8 * k);
        }
      }
      st[i] = v;
    }
  } else {
    const float* src = (const float*)base + (int64_t)img * pitch_n;
    const int64_t plane = (int64_t)H * W;
    for (int i = t; i < MT_STAGE_WORDS; i += MT_THREADS) {
      const int r = i / MT_ROW_WORDS, w = i - r * MT_ROW_WORDS;
      const int y = y0 + r;
      uint32_t v = 0;
      if (y < H) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int e = 4 * w + k;  // byte of the staged row: pixel e / 3, channel e % 3
          const int px = e / 3, c = e - 3 * px;
          const int x = x0 + px;
          if (x < W) v |= frame_u8(src[(int64_t)c * plane + (int64_t)y * W + x]) << (8 * k);
        }
      }
      st[i] = v;
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(MT_THREADS) void frame_metrics_tile_kernel(const seva_metrics_desc d, const MetricsWeights wt,
                                                                        const int tiles_x, const int tiles, double* ssim_part,
                                                                        uint32_t* sse_part) {
  __shared__ uint32_t st[2][MT_STAGE_WORDS];
  __shared__ float hp[5][MT_HALO][MT_TILE];
  __shared__ double red_s[MT_THREADS];
  __shared__ uint32_t red_e[MT_THREADS];

  const int t = threadIdx.x;
  const int img = blockIdx.x / tiles;
  const int tile = blockIdx.x - img * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y0 = ty * MT_TILE, x0 = tx * MT_TILE;
  const int H = d.H, W = d.W;

  stage_frame<KIND>(st[0], d.a, d.a_pitch_n, img, H, W, y0, x0);
  stage_frame<KIND>(st[1], d.b, d.b_pitch_n, img, H, W, y0, x0);
  __syncthreads();
  const uint8_t* sa = (const uint8_t*)st[0];
  const uint8_t* sb = (const uint8_t*)st[1];

  // squared error of the tile's own 32 x 32 pixels (staged bytes outside the image are 0 in both frames)
  uint32_t sse = 0;
  for (int i = t; i < MT_TILE * MT_TILE * 3; i += MT_THREADS) {
    const int r = i / (MT_TILE * 3), c = i - r * (MT_TILE * 3);
    const int df = (int)sa[r * MT_ROW_BYTES + c] - (int)sb[r * MT_ROW_BYTES + c];
    sse += (uint32_t)(df * df);
  }

  double ssum = 0.0;
  const int vh = H - (MT_WIN - 1), vw = W - (MT_WIN - 1);  // valid positions
  if (d.ssim && y0 < vh && x0 < vw) {                      // (uniform over the workgroup)
    const float C1 = 6.5025f, C2 = 58.5225f;               // (0.01 * 255)^2, (0.03 * 255)^2
    const int ox = t & (MT_TILE - 1), og = t >> 5;         // this thread's column and group of 4 rows in the vertical pass
    for (int c = 0; c < 3; ++c) {
      for (int i = t; i < MT_HALO * MT_TILE; i += MT_THREADS) {
        const int r = i >> 5, o = i & (MT_TILE - 1);
        const uint8_t* pa = sa + r * MT_ROW_BYTES + o * 3 + c;
        const uint8_t* pb = sb + r * MT_ROW_BYTES + o * 3 + c;
        float hx = 0.f, hy = 0.f, hxx = 0.f, hyy = 0.f, hxy = 0.f;
#pragma unroll
        for (int k = 0; k < MT_WIN; ++k) {
          const float x = (float)pa[3 * k], y = (float)pb[3 * k];
          const float g = wt.g[k];
          hx = __fadd_rn(hx, __fmul_rn(g, x));
          hy = __fadd_rn(hy, __fmul_rn(g, y));
          hxx = __fadd_rn(hxx, __fmul_rn(g, __fmul_rn(x, x)));
          hyy = __fadd_rn(hyy, __fmul_rn(g, __fmul_rn(y, y)));
          hxy = __fadd_rn(hxy, __fmul_rn(g, __fmul_rn(x, y)));
        }
        hp[0][r][o] = hx;
        hp[1][r][o] = hy;
        hp[2][r][o] = hxx;
        hp[3][r][o] = hyy;
        hp[4][r][o] = hxy;
      }
      __syncthreads();
      float m[5][4];
#pragma unroll
      for (int p = 0; p < 5; ++p) {
        float col[MT_WIN + 3];
#pragma unroll
        for (int i = 0; i < MT_WIN + 3; ++i) col[i] = hp[p][og * 4 + i][ox];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float acc = 0.f;
#pragma unroll
          for (int k = 0; k < MT_WIN; ++k) acc = __fadd_rn(acc, __fmul_rn(wt.g[k], col[j + k]));
          m[p][j] = acc;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int oy = y0 + og * 4 + j, oxg = x0 + ox;
        if (oy < vh && oxg < vw) {
          const float mx = m[0][j], my = m[1][j];
          const float mxx = __fmul_rn(mx, mx), myy = __fmul_rn(my, my), mxy = __fmul_rn(mx, my);
          const float sx = __fsub_rn(m[2][j], mxx), sy = __fsub_rn(m[3][j], myy), sxy = __fsub_rn(m[4][j], mxy);
          const float num = __fmul_rn(__fadd_rn(__fmul_rn(2.0f, mxy), C1), __fadd_rn(__fmul_rn(2.0f, sxy), C2));
          const float den = __fmul_rn(__fadd_rn(__fadd_rn(mxx, myy), C1), __fadd_rn(__fadd_rn(sx, sy), C2));
          const float v = __fdiv_rn(num, den);
          if (d.ssim_map) d.ssim_map[(((int64_t)img * 3 + c) * vh + oy) * vw + oxg] = v;
          ssum += (double)v;
        }
      }
      __syncthreads();  // hp is rewritten by the next channel
    }
  }

  using P = Pair<double, uint32_t>;
  const P r = block_tree<MT_THREADS>(P{ssum, sse}, PairRed<double, uint32_t>{red_s, red_e}, [](P x, P y) { return P{x.a + y.a, x.b + y.b}; });
  if (t == 0) {
    sse_part[blockIdx.x] = r.b;
    if (d.ssim) ssim_part[blockIdx.x] = r.a;
  }
}

// one workgroup per image folds its row of the slab
__global__ __launch_bounds__(MT_THREADS) void frame_metrics_sum_kernel(const double* __restrict__ ssim_part,
                                                                       const uint32_t* __restrict__ sse_part, int tiles,
                                                                       int64_t* __restrict__ sse, double* __restrict__ ssim_sum) {
  __shared__ double red_s[MT_THREADS];
  __shared__ unsigned long long red_e[MT_THREADS];
  const int t = threadIdx.x, img = blockIdx.x;
  using P = Pair<double, unsigned long long>;
  const auto part = [&](int i) {  // (the SSIM partials exist only where SSIM was asked for)
    const int64_t k = (int64_t)img * tiles + i;
    return P{ssim_sum ? ssim_part[k] : 0.0, sse_part[k]};
  };
  const P r = slab_fold<MT_THREADS>(P{0.0, 0}, tiles, part, PairRed<double, unsigned long long>{red_s, red_e},
                                    [](P x, P y) { return P{x.a + y.a, x.b + y.b}; });
  if (t == 0) {
    sse[img] = (int64_t)r.b;
    if (ssim_sum) ssim_sum[img] = r.a;
  }
}

inline int64_t metrics_tiles(int32_t H, int32_t W) {
  return (int64_t)((H + MT_TILE - 1) / MT_TILE) * ((W + MT_TILE - 1) / MT_TILE);
}

}  // namespace

extern "C" int seva_frame_metrics_size(int32_t n, int32_t H, int32_t W, int64_t* workspace_bytes) {
  SEVA_REQUIRE(n > 0 && H > 0 && W > 0 && workspace_bytes, "frame_metrics_size: bad arguments n=%d H=%d W=%d", n, H, W);
  *workspace_bytes = (int64_t)n * metrics_tiles(H, W) * 12;  // fp64 SSIM partials, then u32 SSE partials
  return SEVA_OK;
}

extern "C" int seva_frame_metrics(const seva_metrics_desc* d, seva_stream_t stream) {
  SEVA_REQUIRE(d && d->a && d->b && d->sse && d->workspace, "frame_metrics: null descriptor, a, b, sse or workspace");
  SEVA_REQUIRE(d->n > 0 && d->H > 0 && d->W > 0, "frame_metrics: bad sizes n=%d H=%d W=%d", d->n, d->H, d->W);
  if (int rc = frame_checks("frame_metrics", d->kind, d->H, d->W, d->a, d->a_pitch_n, d->b, d->b_pitch_n)) return rc;
  const int64_t elems = 3 * (int64_t)d->H * d->W;
  SEVA_REQUIRE(d->ssim || (!d->ssim_sum && !d->ssim_map), "frame_metrics: ssim_sum / ssim_map given without ssim");
  if (d->ssim) {
    SEVA_REQUIRE(d->ssim_sum, "frame_metrics: ssim needs ssim_sum");
    SEVA_REQUIRE(d->H >= MT_WIN && d->W >= MT_WIN, "frame_metrics: SSIM needs H, W >= 11 (the 11 x 11 window), got %d x %d", d->H, d->W);
  }
  const int64_t tiles = metrics_tiles(d->H, d->W);
  const int64_t blocks = (int64_t)d->n * tiles;
  SEVA_REQUIRE(grid_fits(blocks), "frame_metrics: n * tiles = %lld exceeds the grid", (long long)blocks);
  SEVA_REQUIRE(d->workspace_bytes >= blocks * 12 && (((uintptr_t)d->workspace) & 7) == 0,
               "frame_metrics: workspace of %lld bytes (need %lld, 8-byte aligned)", (long long)d->workspace_bytes, (long long)(blocks * 12));

  // g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in fp64, rounded once to fp32
  MetricsWeights wt;
  double g[MT_WIN], sum = 0.0;
  for (int k = 0; k < MT_WIN; ++k) {
    g[k] = exp(-(double)((k - 5) * (k - 5)) / 4.5);
    sum += g[k];
  }
  for (int k = 0; k < MT_WIN; ++k) wt.g[k] = (float)(g[k] / sum);

  double* ssim_part = (double*)d->workspace;
  uint32_t* sse_part = (uint32_t*)((char*)d->workspace + blocks * 8);
  const int tiles_x = (d->W + MT_TILE - 1) / MT_TILE;
  hipStream_t s = (hipStream_t)stream;
  SevaProfScope prof(4, (double)d->n * elems * (d->kind == FRAME_U8 ? 2.0 : 8.0), s);
  if (d->kind == FRAME_U8)
    hipLaunchKernelGGL(frame_metrics_tile_kernel<FRAME_U8>, dim3((unsigned)blocks), dim3(MT_THREADS), 0, s, *d, wt, tiles_x, (int)tiles,
                       ssim_part, sse_part);
  else
    hipLaunchKernelGGL(frame_metrics_tile_kernel<FRAME_F32>, dim3((unsigned)blocks), dim3(MT_THREADS), 0, s, *d, wt, tiles_x, (int)tiles,
                       ssim_part, sse_part);
  if (int rc = seva_check_launch("frame_metrics_tile_kernel")) return rc;
  hipLaunchKernelGGL(frame_metrics_sum_kernel, dim3((unsigned)d->n), dim3(MT_THREADS), 0, s, ssim_part, sse_part, (int)tiles, d->sse,
                     d->ssim ? d->ssim_sum : (double*)nullptr);
  return seva_check_launch("frame_metrics_sum_kernel");
}
