// Dynamic-range audit of one tensor: exact exponent histogram, zero / inf / NaN / at-max counts and the finite extrema of |x|, in
// one streaming pass (seva_tensor_range; the 72-word contract is in include/seva_hip.h).  Everything is an integer test on the
// element's bit pattern: no floating-point instruction touches a streamed value, so denormal-flush modes cannot change a count.
//
// Counting scheme: lane-private counters.  A 256-thread workgroup owns [68 words][256 threads] u32 in LDS (68 KiB, 17 KiB per
// wave, two workgroups per CU); thread t only ever touches column t, whose bank is t mod 64 whatever the word, so the increments
// of a wave never meet on a bank or on an address -- activations pile into three or four bins, which a shared per-wave histogram
// would serialise on.  The common case (a normal value inside the table, below the format's maximum) is one compare, one
// address and one LDS increment per element plus max / min on the magnitude bits; zeros, subnormals, the clamped ends of the
// f32 table, the format's maximum and non-finite values take a divergent slow path.  The extrema are kept as magnitude bits of the
// tensor's own format (their integer order is the order of |x|) and turned into f32 bit patterns once, by the second kernel.
//
// Work split: the tensor is cut into units -- 16-byte vectors where base and pitch allow them (the vectors of a row; a dense
// tensor is one long row and may end in a partial vector, read element by element), single elements otherwise.  Workgroup w
// takes the units of elements [w * share, (w + 1) * share), 64-bit indices throughout.  Each workgroup flushes its table to
// workspace[w][72]; a second kernel (one workgroup per word) folds the partial tables (slab_fold, frame_common.h; the extrema go
// through the same fixed tree).  No global atomics; the counts are integers, so the result does not depend on how the tensor was cut.
#include "frame_common.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_WORDS = SEVA_RANGE_WORDS;         // 72
constexpr int RG_SLOTS = 68;                       // words 0 .. 67 are counts
constexpr int RG_UNROLL = 4;                       // units a thread has in flight
constexpr int64_t RG_SHARE = SEVA_RANGE_WG_ELEMS;  // elements per workgroup (a multiple of it for tensors above RG_SHARE * RG_MAX_WGS)
constexpr int64_t RG_MAX_WGS = SEVA_RANGE_MAX_WGS;
constexpr int W_ZERO = 0, W_INF = 65, W_NAN = 66, W_ATMAX = 67, W_MAXABS = 68, W_MINABS = 69, W_TOTAL = 70;

template <int DT>
struct Fmt;
template <>
struct Fmt<SEVA_RANGE_F32> {
  static constexpr int BYTES = 4, VE = 4;
};
template <>
struct Fmt<SEVA_RANGE_F16> {
  static constexpr int BYTES = 2, VE = 8;
};
template <>
struct Fmt<SEVA_RANGE_E4M3> {
  static constexpr int BYTES = 1, VE = 16;
};

struct Acc {
  uint32_t* col;  // this thread's column of the LDS table: col[word * RG_THREADS]
  uint32_t mx;    // largest finite magnitude bits seen (0: none)
  uint32_t mn;    // smallest finite non-zero magnitude bits seen (0xFFFFFFFF: none)
};

// one LDS add without return on an address no other lane uses (fire and forget: no read-wait-write chain per element)
__device__ __forceinline__ void bump(const Acc& a, uint32_t word) {
  __hip_atomic_fetch_add(a.col + word * RG_THREADS, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// `m`: the element's magnitude bits in its own format.  Word numbering is the contract's: bin k = e + 32 is word 1 + k.
template <int DT>
__device__ __forceinline__ void count(Acc& a, uint32_t m) {
  if (DT == SEVA_RANGE_F16) {
    if (__builtin_expect(m - 0x0400u < 0x77FFu, 1)) {  // normal and below 65504: e = E - 15
      bump(a, (m >> 10) + 18);
      a.mx = max(a.mx, m);
      a.mn = min(a.mn, m);
    } else if (m == 0) {
      bump(a, W_ZERO);
    } else if (m < 0x0400u) {  // subnormal: m * 2^-24, e = msb(m) - 24
      bump(a, 40 - __clz(m));
      a.mx = max(a.mx, m);
      a.mn = min(a.mn, m);
    } else if (m == 0x7BFFu) {
      bump(a, 48);
      bump(a, W_ATMAX);
      a.mx = max(a.mx, m);
      a.mn = min(a.mn, m);
    } else {
      bump(a, m == 0x7C00u ? W_INF : W_NAN);
    }
  } else if (DT == SEVA_RANGE_E4M3) {
    if (__builtin_expect(m - 8u < 0x76u, 1)) {  // normal and below 448: e = E - 7
      bump(a, (m >> 3) + 26);
      a.mx = max(a.mx, m);
      a.mn = min(a.mn, m);
    } else if (m == 0) {
      bump(a, W_ZERO);
    } else if (m < 8u) {  // subnormal: m * 2^-9, e = msb(m) - 9
      bump(a, 55 - __clz(m));
      a.mx = max(a.mx, m);
      a.mn = min(a.mn, m);
    } else if (m == 0x7Eu) {
      bump(a, 41);
      bump(a, W_ATMAX);
      a.mx = max(a.mx, m);
      a.mn = min(a.mn, m);
    } else {  // 0x7F: the encoding has no infinity
      bump(a, W_NAN);
    }
  } else {
    const uint32_t rel = m - (95u << 23);  // e in [-32, 31] <=> rel < 64 << 23
    if (__builtin_expect(rel < (64u << 23), 1)) {
      bump(a, (rel >> 23) + 1);
      a.mx = max(a.mx, m);
      a.mn = min(a.mn, m);
    } else if (m == 0) {
      bump(a, W_ZERO);
    } else if (m < 0x7F800000u) {  // finite outside the table: clamped to its first / last bin (subnormals: E = 0)
      bump(a, m < (95u << 23) ? 1 : 64);
      if (m == 0x7F7FFFFFu) bump(a, W_ATMAX);
      a.mx = max(a.mx, m);
      a.mn = min(a.mn, m);
    } else {
      bump(a, m == 0x7F800000u ? W_INF : W_NAN);
    }
  }
}

template <int DT>
__device__ __forceinline__ void count_dword(Acc& a, uint32_t w) {
  if (DT == SEVA_RANGE_F32) {
    count<DT>(a, w & 0x7FFFFFFFu);
  } else if (DT == SEVA_RANGE_F16) {
    count<DT>(a, w & 0x7FFFu);
    count<DT>(a, (w >> 16) & 0x7FFFu);
  } else {
#pragma unroll
    for (int b = 0; b < 4; ++b) count<DT>(a, (w >> (8 * b)) & 0x7Fu);
  }
}

template <int DT>
__device__ __forceinline__ void count_scalar(Acc& a, const char* p) {
  if (DT == SEVA_RANGE_F32)
    count<DT>(a, *(const uint32_t*)p & 0x7FFFFFFFu);
  else if (DT == SEVA_RANGE_F16)
    count<DT>(a, (uint32_t)*(const uint16_t*)p & 0x7FFFu);
  else
    count<DT>(a, (uint32_t)*(const uint8_t*)p & 0x7Fu);
}

// magnitude bits of the format -> f32 bit pattern of the same value (exact: every f16 and e4m3 value is an f32)
__device__ __forceinline__ uint32_t to_f32_bits(int dt, uint32_t m) {
  if (dt == SEVA_RANGE_F16) {
    if (m >= 0x0400u) return (m << 13) + 0x38000000u;
    return __float_as_uint(__uint2float_rn(m)) - (24u << 23);  // m in 1 .. 1023: an exact, normal float, times 2^-24
  }
  if (dt == SEVA_RANGE_E4M3) {
    if (m >= 8u) return (m << 20) + 0x3C000000u;
    return __float_as_uint(__uint2float_rn(m)) - (9u << 23);
  }
  return m;
}

// VEC: units are 16-byte vectors of a row (upr = ceil(cols / VE) per row); otherwise single elements (upr = cols).
template <int DT, bool VEC>
__global__ __launch_bounds__(RG_THREADS) void tensor_range_kernel(const char* __restrict__ x, const int64_t rows, const int64_t cols,
                                                                  const int64_t pitch, const int64_t upr, const int64_t units,
                                                                  const int64_t wg_units, uint64_t* __restrict__ part) {
  constexpr int VE = VEC ? Fmt<DT>::VE : 1;
  constexpr int EB = Fmt<DT>::BYTES;
  __shared__ uint32_t tab[RG_SLOTS * RG_THREADS];
  const int t = threadIdx.x;
  for (int i = t; i < RG_SLOTS * RG_THREADS; i += RG_THREADS) tab[i] = 0;  // (column t only: no barrier needed before counting)
  Acc acc{tab + t, 0u, 0xFFFFFFFFu};

  const int64_t u0 = (int64_t)blockIdx.x * wg_units;
  const int64_t u1 = min(units, u0 + wg_units);
  // this thread's units: u0 + t, + 256, ...; (r, v) = (row, unit of the row) advance without a division per unit
  const int64_t qs = RG_THREADS / upr, rs = RG_THREADS % upr;  // (uniform)
  int64_t u = u0 + t;
  int64_t r = u / upr, v = u - r * upr;
  while (u < u1) {
    const char* p[RG_UNROLL];
    int n[RG_UNROLL];  // elements of the unit; 0: past the end
    uint4 q[RG_UNROLL];
#pragma unroll
    for (int j = 0; j < RG_UNROLL; ++j) {
      n[j] = 0;
      if (u < u1) {
        const int64_t c0 = v * VE;
        p[j] = x + (r * pitch + c0) * EB;
        n[j] = (int)min((int64_t)VE, cols - c0);
        if (VEC && n[j] == VE) q[j] = *(const uint4*)p[j];
      }
      u += RG_THREADS;
      r += qs;
      v += rs;
      if (v >= upr) {
        v -= upr;
        ++r;
      }
    }
#pragma unroll
    for (int j = 0; j < RG_UNROLL; ++j) {
      if (VEC && n[j] == VE) {
        count_dword<DT>(acc, q[j].x);
        count_dword<DT>(acc, q[j].y);
        count_dword<DT>(acc, q[j].z);
        count_dword<DT>(acc, q[j].w);
      } else {
        for (int e = 0; e < n[j]; ++e) count_scalar<DT>(acc, p[j] + e * EB);
      }
    }
  }
  __syncthreads();

  // flush: wave w adds words w, w + 4, ... over the 256 columns; then the extrema through the (now free) first two rows
  const int lane = t & 63, wave = t >> 6;
  uint64_t* out = part + (int64_t)blockIdx.x * RG_WORDS;
  for (int w = wave; w < RG_SLOTS; w += RG_THREADS / 64) {
    uint64_t s = 0;
#pragma unroll
    for (int j = 0; j < RG_THREADS / 64; ++j) s += tab[w * RG_THREADS + lane + 64 * j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out[w] = s;
  }
  __syncthreads();
  using P = Pair<uint32_t, uint32_t>;  // (max, min)
  const P ext = block_tree<RG_THREADS>(P{acc.mx, acc.mn}, PairRed<uint32_t, uint32_t>{tab, tab + RG_THREADS},
                                       [](P x, P y) { return P{x.a > y.a ? x.a : y.a, x.b < y.b ? x.b : y.b}; });
  if (t == 0) {
    out[W_MAXABS] = ext.a;
    out[W_MINABS] = ext.b;
    out[W_TOTAL] = 0;
    out[W_TOTAL + 1] = 0;
  }
}

// one workgroup per output word folds that word of the partial tables
__global__ __launch_bounds__(RG_THREADS) void tensor_range_sum_kernel(const uint64_t* __restrict__ part, const int64_t wgs, const int dt,
                                                                      const uint64_t total, uint64_t* __restrict__ out) {
  __shared__ uint64_t red[RG_THREADS];
  const int t = threadIdx.x, w = blockIdx.x;
  if (w >= W_TOTAL) {
    if (t == 0) out[w] = w == W_TOTAL ? total : 0;
    return;
  }
  const bool is_max = w == W_MAXABS, is_min = w == W_MINABS;  // (uniform over the workgroup)
  const auto op = [=](uint64_t a, uint64_t b) { return is_max ? (a > b ? a : b) : is_min ? (a < b ? a : b) : a + b; };
  uint64_t r = slab_fold<RG_THREADS>((uint64_t)(is_min ? 0xFFFFFFFFull : 0), wgs, [&](int64_t i) { return part[i * RG_WORDS + w]; }, red, op);
  if (t == 0) {
    if (is_max) r = r ? to_f32_bits(dt, (uint32_t)r) : 0;
    if (is_min) r = r != 0xFFFFFFFFull ? to_f32_bits(dt, (uint32_t)r) : 0x7F800000ull;
    out[w] = r;
  }
}

// elements per workgroup and number of workgroups of a tensor of `total` elements
inline void range_split(int64_t total, int64_t* share, int64_t* wgs) {
  int64_t s = RG_SHARE;
  if (total > RG_SHARE * RG_MAX_WGS) s = ((total + RG_MAX_WGS - 1) / RG_MAX_WGS + RG_SHARE - 1) / RG_SHARE * RG_SHARE;
  *share = s;
  *wgs = (total + s - 1) / s;
}

template <int DT>
int range_launch(const seva_range_desc* d, int64_t rows, int64_t cols, int64_t pitch, bool vec, int64_t share, int64_t wgs, hipStream_t s) {
  const int64_t upr = vec ? (cols + Fmt<DT>::VE - 1) / Fmt<DT>::VE : cols;
  const int64_t units = rows * upr;
  const int64_t wg_units = vec ? share / Fmt<DT>::VE : share;
  // (rows * cols == units * VE, or one row with a ragged last vector: the units of elements [w * share, ..) are [w * wg_units, ..))
  const int64_t blocks = (units + wg_units - 1) / wg_units;
  if (blocks != wgs) {
    seva_set_error("tensor_range: internal split mismatch (%lld workgroups for %lld partial tables)", (long long)blocks, (long long)wgs);
    return SEVA_ERR_ARG;
  }
  if (vec)
    hipLaunchKernelGGL((tensor_range_kernel<DT, true>), dim3((unsigned)wgs), dim3(RG_THREADS), 0, s, (const char*)d->x, rows, cols, pitch,
                       upr, units, wg_units, (uint64_t*)d->workspace);
  else
    hipLaunchKernelGGL((tensor_range_kernel<DT, false>), dim3((unsigned)wgs), dim3(RG_THREADS), 0, s, (const char*)d->x, rows, cols, pitch,
                       upr, units, wg_units, (uint64_t*)d->workspace);
  return seva_check_launch("tensor_range_kernel");
}

}  // namespace

extern "C" int seva_tensor_range_size(int64_t rows, int64_t cols, int64_t* workspace_bytes) {
  SEVA_REQUIRE(rows > 0 && cols > 0 && workspace_bytes, "tensor_range_size: bad arguments rows=%lld cols=%lld", (long long)rows, (long long)cols);
  SEVA_REQUIRE(rows <= (1ll << 46) / cols, "tensor_range_size: rows * cols = %lld * %lld exceeds 2^46 elements", (long long)rows, (long long)cols);
  int64_t share, wgs;
  range_split(rows * cols, &share, &wgs);
  *workspace_bytes = wgs * RG_WORDS * 8;
  return SEVA_OK;
}

extern "C" int seva_tensor_range(const seva_range_desc* d, seva_stream_t stream) {
  SEVA_REQUIRE(d && d->x && d->out && d->workspace, "tensor_range: null descriptor, x, out or workspace");
  SEVA_REQUIRE(d->dtype == SEVA_RANGE_F32 || d->dtype == SEVA_RANGE_F16 || d->dtype == SEVA_RANGE_E4M3,
               "tensor_range: dtype=%d (0: f32, 1: f16, 2: e4m3)", d->dtype);
  SEVA_REQUIRE(d->rows > 0 && d->cols > 0 && d->pitch >= d->cols, "tensor_range: bad sizes rows=%lld cols=%lld pitch=%lld",
               (long long)d->rows, (long long)d->cols, (long long)d->pitch);
  SEVA_REQUIRE(d->rows <= (1ll << 46) / d->cols, "tensor_range: rows * cols = %lld * %lld exceeds 2^46 elements", (long long)d->rows,
               (long long)d->cols);
  const int eb = d->dtype == SEVA_RANGE_F32 ? 4 : d->dtype == SEVA_RANGE_F16 ? 2 : 1;
  SEVA_REQUIRE((((uintptr_t)d->x) & (uintptr_t)(eb - 1)) == 0, "tensor_range: x is not aligned to its %d-byte elements", eb);
  SEVA_REQUIRE(((((uintptr_t)d->out) | ((uintptr_t)d->workspace)) & 7) == 0, "tensor_range: out and workspace must be 8-byte aligned");
  const int64_t total = d->rows * d->cols;
  int64_t share, wgs;
  range_split(total, &share, &wgs);
  SEVA_REQUIRE(d->workspace_bytes >= wgs * RG_WORDS * 8, "tensor_range: workspace of %lld bytes (need %lld)", (long long)d->workspace_bytes,
               (long long)(wgs * RG_WORDS * 8));

  // a dense tensor is one long row; 16-byte vectors need an aligned base, rows a whole number of vectors apart, and rows that
  // are a whole number of vectors long (one row may end in a ragged vector)
  int64_t rows = d->rows, cols = d->cols, pitch = d->pitch;
  if (pitch == cols || rows == 1) {
    cols = total;
    rows = 1;
    pitch = cols;
  }
  const int ve = 16 / eb;
  const bool vec = (((uintptr_t)d->x) & 15) == 0 && (rows == 1 || (pitch % ve == 0 && cols % ve == 0));
  hipStream_t s = (hipStream_t)stream;
  // (no SevaProfScope: the audit's traffic is not booked into the profile of the step it audits)
  int rc;
  if (d->dtype == SEVA_RANGE_F32)
    rc = range_launch<SEVA_RANGE_F32>(d, rows, cols, pitch, vec, share, wgs, s);
  else if (d->dtype == SEVA_RANGE_F16)
    rc = range_launch<SEVA_RANGE_F16>(d, rows, cols, pitch, vec, share, wgs, s);
  else
    rc = range_launch<SEVA_RANGE_E4M3>(d, rows, cols, pitch, vec, share, wgs, s);
  if (rc) return rc;
  hipLaunchKernelGGL(tensor_range_sum_kernel, dim3(RG_WORDS), dim3(RG_THREADS), 0, s, (const uint64_t*)d->workspace, wgs, (int)d->dtype,
                     (uint64_t)total, d->out);
  return seva_check_launch("tensor_range_sum_kernel");
}
