// Image front and back end: pictures -> [-1, 1] fp32 frames (load_img_and_K / transform_img_and_K of the reference's
// seva/eval.py) and decoded frames -> uint8 (save_output).  Memory-bound elementwise kernels, one thread per output pixel
// (all three channels).  The arithmetic contract is in include/seva_hip.h: every fp32 operation is rounded on its own.  The
// file is built with -ffp-contract=off AND spells each operation as __fadd_rn / __fmul_rn / __fdiv_rn, so no FMA and no
// reciprocal-multiply can form whatever the flags are.  The uint8 rule itself (frame_u8) is in frame_common.h, shared with the scores.
#include "frame_common.h"

namespace {

constexpr int FR_THREADS = 256;

inline unsigned fr_grid(int64_t work) {
  int64_t b = (work + FR_THREADS - 1) / FR_THREADS;
  if (b < 1) b = 1;
  if (b > 16384) b = 16384;
  return (unsigned)b;
}

enum { SRC_U8_RGB = 0, SRC_U8_RGBA = 1, SRC_F32 = 2 };

// one source pixel as the three fp32 values the reference resizes
template <int KIND>
__device__ __forceinline__ void load_pixel(const seva_image_desc& d, int img, int yy, int xx, float& r, float& g, float& b) {
  if (KIND == SRC_F32) {
    const float* p = (const float*)d.src + (int64_t)img * d.src_pitch_n + (int64_t)yy * d.src_pitch_row + xx;
    r = p[0];
    g = p[d.src_pitch_c];
    b = p[2 * d.src_pitch_c];
  } else if (KIND == SRC_U8_RGB) {
    const uint8_t* p = (const uint8_t*)d.src + (int64_t)img * d.src_pitch_n + (int64_t)yy * d.src_pitch_row + (int64_t)xx * 3;
    r = __fdiv_rn((float)p[0], 255.0f);
    g = __fdiv_rn((float)p[1], 255.0f);
    b = __fdiv_rn((float)p[2], 255.0f);
  } else {
    const uint8_t* p = (const uint8_t*)d.src + (int64_t)img * d.src_pitch_n + (int64_t)yy * d.src_pitch_row + (int64_t)xx * 4;
    const uint32_t px = *(const uint32_t*)p;  // R | G << 8 | B << 16 | A << 24
    const float a = __fdiv_rn((float)(px >> 24), 255.0f);
    const float na = __fsub_rn(1.0f, a);
    float b0 = 1.0f, b1 = 1.0f, b2 = 1.0f;
    if (d.context_rgb) {
      const float* c = d.context_rgb + ((int64_t)yy * d.w + xx) * 3;
      b0 = c[0]; b1 = c[1]; b2 = c[2];
    }
    r = __fadd_rn(__fmul_rn(__fdiv_rn((float)(px & 255u), 255.0f), a), __fmul_rn(b0, na));
    g = __fadd_rn(__fmul_rn(__fdiv_rn((float)((px >> 8) & 255u), 255.0f), a), __fmul_rn(b1, na));
    b = __fadd_rn(__fmul_rn(__fdiv_rn((float)((px >> 16) & 255u), 255.0f), a), __fmul_rn(b2, na));
  }
}

template <int KIND>
__global__ void image_area_crop_kernel(const seva_image_desc d, const int affine) {
  const int64_t plane = (int64_t)d.H * d.W;
  const int64_t total = (int64_t)d.n * plane;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int img = (int)(i / plane);
    const int64_t pix = i - (int64_t)img * plane;
    const int y = (int)(pix / d.W), x = (int)(pix - (int64_t)y * d.W);
    const int ry = d.ct + y, rx = d.cl + x;  // position in the resized image
    float r = d.pad_value, g = d.pad_value, b = d.pad_value;
    if (ry >= 0 && ry < d.rh && rx >= 0 && rx < d.rw) {
      const int y0 = (int)(((int64_t)ry * d.h) / d.rh), y1 = (int)((((int64_t)ry + 1) * d.h + d.rh - 1) / d.rh);
      const int x0 = (int)(((int64_t)rx * d.w) / d.rw), x1 = (int)((((int64_t)rx + 1) * d.w + d.rw - 1) / d.rw);
      float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
      for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) {
          float p0, p1, p2;
          load_pixel<KIND>(d, img, yy, xx, p0, p1, p2);
          s0 = __fadd_rn(s0, p0);
          s1 = __fadd_rn(s1, p1);
          s2 = __fadd_rn(s2, p2);
        }
      const float kh = (float)(y1 - y0), kw = (float)(x1 - x0);
      r = __fdiv_rn(__fdiv_rn(s0, kh), kw);
      g = __fdiv_rn(__fdiv_rn(s1, kh), kw);
      b = __fdiv_rn(__fdiv_rn(s2, kh), kw);
    }
    if (affine) {
      r = __fadd_rn(__fmul_rn(r, d.out_mul), d.out_add);
      g = __fadd_rn(__fmul_rn(g, d.out_mul), d.out_add);
      b = __fadd_rn(__fmul_rn(b, d.out_mul), d.out_add);
    }
    float* o = d.out + (int64_t)img * d.out_pitch_n + pix;
    o[0] = r;
    o[plane] = g;
    o[2 * plane] = b;
  }
}

// One thread per group of 4 consecutive pixels of one image: 12 output bytes = three 32-bit stores where the image's output
// starts 4-byte aligned (it does for every image when H*W*3 % 4 == 0), byte stores otherwise and in an image's last, partial group.
__global__ void rgb_to_u8_kernel(const float* __restrict__ x, int64_t x_pitch_n, uint8_t* __restrict__ out, int n, int64_t plane) {
  const int64_t groups = (plane + 3) >> 2;
  const int64_t total = (int64_t)n * groups;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int img = (int)(i / groups);
    const int64_t p0 = (i - (int64_t)img * groups) << 2;
    const float* s = x + (int64_t)img * x_pitch_n + p0;
    uint8_t* o = out + ((int64_t)img * plane + p0) * 3;
    const int cnt = (int)(plane - p0 < 4 ? plane - p0 : 4);
    uint32_t v[12];  // byte 3 * pixel + channel
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) v[3 * k + c] = k < cnt ? frame_u8(s[(int64_t)c * plane + k]) : 0u;
    if (cnt == 4 && ((uintptr_t)o & 3) == 0) {
      uint32_t* o4 = (uint32_t*)o;
      o4[0] = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
      o4[1] = v[4] | v[5] << 8 | v[6] << 16 | v[7] << 24;
      o4[2] = v[8] | v[9] << 8 | v[10] << 16 | v[11] << 24;
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
        if (k < 3 * cnt) o[k] = (uint8_t)v[k];
    }
  }
}

int image_common_checks(const seva_image_desc* d, const char* who) {
  SEVA_REQUIRE(d && d->src && d->out, "%s: null descriptor, src or out", who);
  SEVA_REQUIRE(d->n > 0 && d->h > 0 && d->w > 0 && d->rh > 0 && d->rw > 0 && d->H > 0 && d->W > 0,
               "%s: bad sizes n=%d src %dx%d resized %dx%d out %dx%d", who, d->n, d->h, d->w, d->rh, d->rw, d->H, d->W);
  SEVA_REQUIRE(d->out_pitch_n >= 3 * (int64_t)d->H * d->W, "%s: out_pitch_n=%lld < 3*H*W", who, (long long)d->out_pitch_n);
  return SEVA_OK;
}

}  // namespace

#define FR_LAUNCH(kern, work, ...)                                                         \
  do {                                                                                     \
    hipStream_t s_ = (hipStream_t)stream;                                                  \
    hipLaunchKernelGGL(kern, dim3(fr_grid(work)), dim3(FR_THREADS), 0, s_, __VA_ARGS__);   \
    return seva_check_launch(#kern);                                                       \
  } while (0)

extern "C" int seva_image_area_crop_u8(const seva_image_desc* d, seva_stream_t stream) {
  if (int rc = image_common_checks(d, "image_area_crop_u8")) return rc;
  SEVA_REQUIRE(d->src_c == 3 || d->src_c == 4, "image_area_crop_u8: src_c=%d (3 or 4)", d->src_c);
  SEVA_REQUIRE(d->src_pitch_row >= (int64_t)d->w * d->src_c && d->src_pitch_n >= (int64_t)(d->h - 1) * d->src_pitch_row + (int64_t)d->w * d->src_c,
               "image_area_crop_u8: source pitches (row %lld, image %lld) too small", (long long)d->src_pitch_row, (long long)d->src_pitch_n);
  SEVA_REQUIRE(d->src_c == 4 || !d->context_rgb, "image_area_crop_u8: context_rgb needs an alpha channel (src_c = 4)");
  SEVA_REQUIRE(d->src_c == 3 || (((uintptr_t)d->src | (uintptr_t)d->src_pitch_row | (uintptr_t)d->src_pitch_n) & 3) == 0,
               "image_area_crop_u8: RGBA source and its pitches must be 4-byte aligned");
  const int affine = !(d->out_mul == 1.0f && d->out_add == 0.0f);
  const int64_t work = (int64_t)d->n * d->H * d->W;
  SevaProfScope prof(4, (double)d->n * ((double)d->h * d->w * d->src_c + 12.0 * d->H * d->W), (hipStream_t)stream);
  if (d->src_c == 4) FR_LAUNCH(image_area_crop_kernel<SRC_U8_RGBA>, work, *d, affine);
  FR_LAUNCH(image_area_crop_kernel<SRC_U8_RGB>, work, *d, affine);
}

extern "C" int seva_image_area_crop_f32(const seva_image_desc* d, seva_stream_t stream) {
  if (int rc = image_common_checks(d, "image_area_crop_f32")) return rc;
  SEVA_REQUIRE(d->src_c == 3 && !d->context_rgb, "image_area_crop_f32: src_c=%d (3), no context_rgb", d->src_c);
  SEVA_REQUIRE(d->src_pitch_row >= d->w && d->src_pitch_c >= (int64_t)(d->h - 1) * d->src_pitch_row + d->w &&
                   d->src_pitch_n >= 2 * d->src_pitch_c + (int64_t)(d->h - 1) * d->src_pitch_row + d->w,
               "image_area_crop_f32: source pitches (row %lld, plane %lld, image %lld) too small", (long long)d->src_pitch_row,
               (long long)d->src_pitch_c, (long long)d->src_pitch_n);
  const int affine = !(d->out_mul == 1.0f && d->out_add == 0.0f);
  const int64_t work = (int64_t)d->n * d->H * d->W;
  SevaProfScope prof(4, (double)d->n * (12.0 * d->h * d->w + 12.0 * d->H * d->W), (hipStream_t)stream);
  FR_LAUNCH(image_area_crop_kernel<SRC_F32>, work, *d, affine);
}

extern "C" int seva_rgb_to_u8(const float* x, int64_t x_pitch_n, uint8_t* out, int32_t n, int32_t H, int32_t W,
                              seva_stream_t stream) {
  SEVA_REQUIRE(x && out && n > 0 && H > 0 && W > 0, "rgb_to_u8: bad args");
  const int64_t plane = (int64_t)H * W;
  SEVA_REQUIRE(x_pitch_n >= 3 * plane, "rgb_to_u8: x_pitch_n=%lld < 3*H*W", (long long)x_pitch_n);
  SevaProfScope prof(4, (double)n * plane * 15.0, (hipStream_t)stream);
  FR_LAUNCH(rgb_to_u8_kernel, (int64_t)n * ((plane + 3) / 4), x, x_pitch_n, out, n, plane);
}
