// On-device augmentations of the per-batch training chain
// (configs/datamodule/semantic/default.yaml:250-264 and 292-358).
//
// Replaces, one streaming pass per tensor each:
//
//   NAGJitterKey                          src/transforms/data.py:651-721
//   NAGDropoutColumns / NAGDropoutRows    src/transforms/data.py:440-648, src/utils/dropout.py:7-22
//   RandomTiltAndRotate / RandomAnisotropicScale / RandomAxisFlip
//                                         src/transforms/geometry.py:28-245
//   NAGColorAutoContrast / NAGColorDrop   src/transforms/point.py:374-545
//
// The reference composes these from about a hundred small launches per batch and reads a
// decision back to the host at every `if torch.rand(1, device=...) < p` and every
// `torch.where(rand < p)[0]`.  Here every scalar decision (rotation, scale, flip, dropped
// columns, contrast, blend, drop) is drawn on the host and arrives BY VALUE; every per-element
// draw comes from the counter-based generator of rng.hpp:
//
//   counter of an element     its LOGICAL index row * n_cols + col
//   counter of a row decision row
//
// never an address or a thread id, so the values do not depend on stride, alignment, grid size
// or on which load / store route a row takes.
//
//   decision   u = (r >> 8) * 2^-24 in [0, 1), `u < p` in f32 like torch.rand(...) < p
//   noise      the construction of torch.nn.init.trunc_normal_ with u = ((r >> 8) + 0.5) * 2^-24:
//                noise = clamp(sigma * sqrt(2) * erfinv(lo + u * (hi - lo)), -trunc, trunc)
//              lo = 2 Phi(-trunc / sigma) - 1, hi = 2 Phi(trunc / sigma) - 1 from the host (f64).
//              lo + u (hi - lo) is evaluated as mid + half * t with mid = (lo + hi) / 2,
//              half = (hi - lo) / 2 and t = 2u - 1 = (2 (r >> 8) + 1 - 2^24) * 2^-24, an odd
//              integer below 2^24 times a power of two: EXACT in f32, |t| <= 1 - 2^-24, so the
//              argument never rounds to +-1 and the noise is always finite.  trunc <= 0:
//              lo = -1, hi = 1, no clamp; the tail ends at sqrt(2) erfinv(1 - 2^-24) = 5.42 sigma.
//
// Memory: a lane owns 4 consecutive rows of a 3- or 7-column tensor (3 or 7 16-byte accesses
// when the tensor is dense and 16-byte aligned) or 4 consecutive elements of a feature table;
// strided tensors (a column block of a wider x), unaligned bases and the last rows take
// per-element accesses of the SAME values.  One read and one write per element; out may be in.
//
// Arithmetic: f32, no contraction except the fmaf written out below, IEEE division.
#include <math.h>

#include "common.hpp"
#include "rng.hpp"

namespace spt {
namespace augment {

constexpr int THREADS = 256;

enum { FEAT_JITTER = 1, FEAT_COLUMNS = 2, FEAT_ROWS = 4, FEAT_ALL = 7 };
enum { GEO_POS = 0, GEO_NORMAL = 1, GEO_EDGE7 = 2 };
enum { GEO_JITTER = 1, GEO_ROTATE = 2, GEO_SCALE = 4, GEO_FLIP = 8, GEO_ALL = 15 };
enum { COL_JITTER = 1, COL_CONTRAST = 2, COL_DROP = 4, COL_ALL = 7 };
enum { VEC_IN = 1, VEC_OUT = 2 };

struct Noise {
  float s;       // sigma * sqrt(2)
  float mid;     // (lo + hi) / 2
  float half;    // (hi - lo) / 2
  float trunc;
  int clamp;
};

struct Geo {
  float R[9];    // row major: out_i = R[3i] x + R[3i+1] y + R[3i+2] z   (pos @ R.T)
  float s[3];
  float snorm;   // ||s||_2
  int axis;
};

__device__ __forceinline__ float noise_of(uint64_t seed, uint64_t counter, const Noise& q) {
  const uint32_t k = rand32(seed, counter) >> 8;
  const float t = (float)((int32_t)(2u * k + 1u) - (1 << 24)) * 0x1p-24f;   // 2u - 1, exact
  const float a = __fmaf_rn(q.half, t, q.mid);
  float z = q.s * erfinvf(a);
  if (q.clamp) z = fminf(fmaxf(z, -q.trunc), q.trunc);
  return z;
}

static bool make_noise(double sigma, double trunc, double lo, double hi, Noise* q) {
  if (!(sigma > 0.0) || !(lo >= -1.0 && hi <= 1.0 && lo < hi)) return false;
  q->s = (float)(sigma * 1.4142135623730951);
  q->mid = (float)(0.5 * (lo + hi));
  q->half = (float)(0.5 * (hi - lo));
  q->trunc = (float)trunc;
  q->clamp = trunc > 0.0;
  return true;
}

static inline bool dense16(const float* p, int64_t ld, int w) {
  return ld == w && ((uintptr_t)p & 15) == 0;
}

// ---- 4 rows of W columns per lane -------------------------------------------------------------
template <int W>
__device__ __forceinline__ void load_rows(const float* p, int64_t ld, bool vec,
                                          int64_t i0, int np, float* v) {
  if (vec && np == 4) {
    const float4* q = (const float4*)(p + i0 * W);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float4 a = q[j];
      v[4 * j] = a.x; v[4 * j + 1] = a.y; v[4 * j + 2] = a.z; v[4 * j + 3] = a.w;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < W; ++c) v[r * W + c] = r < np ? p[(i0 + r) * ld + c] : 0.0f;
  }
}

template <int W>
__device__ __forceinline__ void store_rows(float* p, int64_t ld, bool vec,
                                           int64_t i0, int np, const float* v) {
  if (vec && np == 4) {
    float4* q = (float4*)(p + i0 * W);
#pragma unroll
    for (int j = 0; j < W; ++j)
      q[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < np) {
#pragma unroll
        for (int c = 0; c < W; ++c) p[(i0 + r) * ld + c] = v[r * W + c];
      }
  }
}

// ---- jitter + column dropout + row dropout of a feature table ---------------------------------
__global__ __launch_bounds__(THREADS) void features_kernel(
    const float* x, float* out, int64_t n, int c, int64_t ld_x, int64_t ld_out, int vec,
    int flags, uint64_t seed_jitter, Noise q, uint64_t col_mask, uint64_t seed_rows,
    float p_rows) {
  const int64_t total = n * c;
  const int64_t groups = (total + 3) >> 2;
  const bool small = total <= 0xFFFFFFFFll;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
    const int64_t e0 = g * 4;
    const int ne = (total - e0) < 4 ? (int)(total - e0) : 4;
    const int64_t row0 = small ? (int64_t)((uint32_t)e0 / (uint32_t)c) : e0 / c;
    const int col0 = (int)(e0 - row0 * c);
    float v[4];
    if ((vec & VEC_IN) && ne == 4) {
      const float4 a = *(const float4*)(x + e0);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
      int64_t row = row0;
      int col = col0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = j < ne ? x[row * ld_x + col] : 0.0f;
        if (++col == c) { col = 0; ++row; }
      }
    }
    {
      int64_t row = row0;
      int col = col0;
      bool drop_row = (flags & FEAT_ROWS) && rand_unit(seed_rows, (uint64_t)row) < p_rows;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (flags & FEAT_JITTER) v[j] = v[j] + noise_of(seed_jitter, (uint64_t)(e0 + j), q);
        if ((flags & FEAT_COLUMNS) && ((col_mask >> col) & 1ull)) v[j] = 0.0f;
        if (drop_row) v[j] = 0.0f;
        if (++col == c) {
          col = 0;
          ++row;
          drop_row = (flags & FEAT_ROWS) && rand_unit(seed_rows, (uint64_t)row) < p_rows;
        }
      }
    }
    if ((vec & VEC_OUT) && ne == 4) {
      *(float4*)(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      int64_t row = row0;
      int col = col0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < ne) out[row * ld_out + col] = v[j];
        if (++col == c) { col = 0; ++row; }
      }
    }
  }
}

// ---- pos / normal / 7-column edge_attr --------------------------------------------------------
// out_i = fma(R[3i+2], z, fma(R[3i+1], y, R[3i] * x))
__device__ __forceinline__ void rotate3(float* v, const Geo& g) {
  const float x = v[0], y = v[1], z = v[2];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    v[i] = __fmaf_rn(g.R[3 * i + 2], z, __fmaf_rn(g.R[3 * i + 1], y, __fmul_rn(g.R[3 * i], x)));
}

__device__ __forceinline__ void scale3(float* v, const Geo& g) {
  v[0] = __fmul_rn(v[0], g.s[0]);
  v[1] = __fmul_rn(v[1], g.s[1]);
  v[2] = __fmul_rn(v[2], g.s[2]);
}

__device__ __forceinline__ void flip3(float* v, int axis) {
  v[0] = axis == 0 ? -v[0] : v[0];
  v[1] = axis == 1 ? -v[1] : v[1];
  v[2] = axis == 2 ? -v[2] : v[2];
}

// normal[normal[:, 2] < 0] *= -1
__device__ __forceinline__ void up3(float* v) {
  if (v[2] < 0.0f) { v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
}

// F.normalize: v / max(||v||, 1e-12), ||v||^2 = fma(z, z, fma(y, y, x * x))
__device__ __forceinline__ void normalize3(float* v) {
  const float ss = __fmaf_rn(v[2], v[2], __fmaf_rn(v[1], v[1], __fmul_rn(v[0], v[0])));
  const float d = fmaxf(__fsqrt_rn(ss), 1e-12f);
  v[0] = __fdiv_rn(v[0], d);
  v[1] = __fdiv_rn(v[1], d);
  v[2] = __fdiv_rn(v[2], d);
}

template <int W, int MODE>
__global__ __launch_bounds__(THREADS) void geometry_kernel(const float* x, float* out, int64_t n,
                                                           int64_t ld_x, int64_t ld_out, int vec,
                                                           int flags, uint64_t seed, Noise q,
                                                           Geo g) {
  const int64_t groups = (n + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < groups; t += stride) {
    const int64_t i0 = t * 4;
    const int np = (n - i0) < 4 ? (int)(n - i0) : 4;
    float v[4 * W];
    load_rows<W>(x, ld_x, vec & VEC_IN, i0, np, v);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* w = v + r * W;
      if (MODE == GEO_POS && (flags & GEO_JITTER)) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          w[c] = w[c] + noise_of(seed, (uint64_t)((i0 + r) * 3 + c), q);
      }
      if (flags & GEO_ROTATE) {
        rotate3(w, g);
        if (MODE == GEO_NORMAL) up3(w);
      }
      if (flags & GEO_SCALE) {
        scale3(w, g);
        if (MODE == GEO_NORMAL) normalize3(w);
        if (MODE == GEO_EDGE7) {
#pragma unroll
          for (int c = 3; c < W; ++c) w[c] = __fmul_rn(w[c], g.snorm);
        }
      }
      if (flags & GEO_FLIP) {
        flip3(w, g.axis);
        if (MODE == GEO_NORMAL) up3(w);
      }
    }
    store_rows<W>(out, ld_out, vec & VEC_OUT, i0, np, v);
  }
}

// ---- colours ----------------------------------------------------------------------------------
// min / max of f32 through integer atomics on the bit patterns: exact and order independent.
// +0 is added first so that -0 orders as +0.
__device__ __forceinline__ void atomic_min_f32(float* a, float v) {
  v = v + 0.0f;
  if (v >= 0.0f) atomicMin((int*)a, __float_as_int(v));
  else atomicMax((unsigned int*)a, __float_as_uint(v));
}

__device__ __forceinline__ void atomic_max_f32(float* a, float v) {
  v = v + 0.0f;
  if (v >= 0.0f) atomicMax((int*)a, __float_as_int(v));
  else atomicMin((unsigned int*)a, __float_as_uint(v));
}

// range6 = {min of column 0..2, max of column 0..2}, preset to {+inf x 3, -inf x 3}.  A NaN in a
// column makes both of its records NaN (Tensor.min / max propagate it): the patterns 0xFFFFFFFF
// and 0x7FFFFFFF are absorbing for the updates above.
__global__ __launch_bounds__(THREADS) void color_range_kernel(const float* c, int64_t n,
                                                             int64_t ld, int vec, int jitter,
                                                             uint64_t seed, Noise q,
                                                             float* range6) {
  __shared__ float s_mn[THREADS / 64][3], s_mx[THREADS / 64][3];
  __shared__ int s_nan[THREADS / 64];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int nan = 0;
  const int64_t groups = (n + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < groups; t += stride) {
    const int64_t i0 = t * 4;
    const int np = (n - i0) < 4 ? (int)(n - i0) : 4;
    float v[12];
    load_rows<3>(c, ld, vec & VEC_IN, i0, np, v);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < np) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          float a = v[r * 3 + k];
          if (jitter) a = a + noise_of(seed, (uint64_t)((i0 + r) * 3 + k), q);
          mn[k] = fminf(mn[k], a);
          mx[k] = fmaxf(mx[k], a);
          if (a != a) nan |= 1 << k;
        }
      }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mn[k] = wave_reduce_min(mn[k]);
    mx[k] = wave_reduce_max(mx[k]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nan |= __shfl_xor(nan, o, 64);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { s_mn[wid][k] = mn[k]; s_mx[wid][k] = mx[k]; }
    s_nan[wid] = nan;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    float a = s_mn[0][k], b = s_mx[0][k];
    int f = s_nan[0];
    for (int w = 1; w < THREADS / 64; ++w) {
      a = fminf(a, s_mn[w][k]);
      b = fmaxf(b, s_mx[w][k]);
      f |= s_nan[w];
    }
    if ((f >> k) & 1) {
      atomicMax((unsigned int*)(range6 + k), 0xFFFFFFFFu);
      atomicMax((int*)(range6 + 3 + k), 0x7FFFFFFF);
    } else {
      // a block without rows keeps +-inf: both are neutral
      atomic_min_f32(range6 + k, a);
      atomic_max_f32(range6 + 3 + k, b);
    }
  }
}

// jitter, then (1 - b) c + b (c - lo) / (hi - lo), then c * 0
__global__ __launch_bounds__(THREADS) void color_kernel(const float* c, float* out, int64_t n,
                                                       int64_t ld_c, int64_t ld_out, int vec,
                                                       int flags, uint64_t seed, Noise q,
                                                       const float* __restrict__ range6,
                                                       float b, float omb) {
  float lo[3] = {0.0f, 0.0f, 0.0f}, den[3] = {1.0f, 1.0f, 1.0f};
  if (flags & COL_CONTRAST) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = range6[k];
      den[k] = range6[3 + k] - lo[k];
    }
  }
  const int64_t groups = (n + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < groups; t += stride) {
    const int64_t i0 = t * 4;
    const int np = (n - i0) < 4 ? (int)(n - i0) : 4;
    float v[12];
    load_rows<3>(c, ld_c, vec & VEC_IN, i0, np, v);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float a = v[r * 3 + k];
        if (flags & COL_JITTER) a = a + noise_of(seed, (uint64_t)((i0 + r) * 3 + k), q);
        if (flags & COL_CONTRAST) {
          const float f = __fdiv_rn(a - lo[k], den[k]);
          a = __fadd_rn(__fmul_rn(omb, a), __fmul_rn(b, f));
        }
        if (flags & COL_DROP) a = __fmul_rn(a, 0.0f);
        v[r * 3 + k] = a;
      }
    store_rows<3>(out, ld_out, vec & VEC_OUT, i0, np, v);
  }
}

}  // namespace augment
}  // namespace spt

using namespace spt;
using namespace spt::augment;

extern "C" int spt_augment_features_f32(const float* x, float* out, int64_t n, int n_cols,
                                        int64_t ld_x, int64_t ld_out, int flags,
                                        uint64_t seed_jitter, double sigma, double trunc,
                                        double lo, double hi, uint64_t col_mask,
                                        uint64_t seed_rows, float p_rows, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(n >= 0 && n_cols >= 1 && n < ((int64_t)1 << 40) && n_cols <= (1 << 20),
                "bad shape");
  SPT_CHECK_ARG(flags >= 1 && flags <= FEAT_ALL, "flags must be a non-empty subset of 1|2|4");
  SPT_CHECK_ARG(ld_x >= n_cols && ld_out >= n_cols, "row stride below n_cols");
  SPT_CHECK_ARG(!(flags & FEAT_COLUMNS) || n_cols <= 64, "column dropout needs n_cols <= 64");
  Noise q{};
  SPT_CHECK_ARG(!(flags & FEAT_JITTER) || make_noise(sigma, trunc, lo, hi, &q),
                "jitter needs sigma > 0 and -1 <= lo < hi <= 1");
  if (n == 0) return 0;
  SPT_CHECK_ARG(x && out, "null pointer");
  SPT_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 3) == 0, "misaligned pointer");
  const int vec = (dense16(x, ld_x, n_cols) ? VEC_IN : 0) | (dense16(out, ld_out, n_cols) ? VEC_OUT : 0);
  const int grid = stream_grid((n * n_cols + 3) >> 2, THREADS);
  features_kernel<<<grid, THREADS, 0, stream>>>(x, out, n, n_cols, ld_x, ld_out, vec, flags,
                                                seed_jitter, q, col_mask, seed_rows, p_rows);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_augment_geometry_f32(const float* x, float* out, int64_t n, int64_t ld_x,
                                        int64_t ld_out, int mode, int flags, uint64_t seed_jitter,
                                        double sigma, double trunc, double lo, double hi,
                                        const float* rotation, const float* scale,
                                        float scale_norm, int flip_axis, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(mode >= GEO_POS && mode <= GEO_EDGE7, "mode must be 0 (pos), 1 (normal) or 2 (edge7)");
  const int w = mode == GEO_EDGE7 ? 7 : 3;
  SPT_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 40), "bad shape");
  SPT_CHECK_ARG(flags >= 1 && flags <= GEO_ALL, "flags must be a non-empty subset of 1|2|4|8");
  SPT_CHECK_ARG(!(flags & GEO_JITTER) || mode == GEO_POS, "jitter is a step of the pos mode only");
  SPT_CHECK_ARG(ld_x >= w && ld_out >= w, "row stride below the column count");
  SPT_CHECK_ARG(!(flags & GEO_ROTATE) || rotation, "rotation is null");
  SPT_CHECK_ARG(!(flags & GEO_SCALE) || scale, "scale is null");
  SPT_CHECK_ARG(!(flags & GEO_FLIP) || (flip_axis >= 0 && flip_axis <= 2), "flip axis out of range");
  Noise q{};
  SPT_CHECK_ARG(!(flags & GEO_JITTER) || make_noise(sigma, trunc, lo, hi, &q),
                "jitter needs sigma > 0 and -1 <= lo < hi <= 1");
  if (n == 0) return 0;
  SPT_CHECK_ARG(x && out, "null pointer");
  SPT_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 3) == 0, "misaligned pointer");
  Geo g{};
  if (flags & GEO_ROTATE) memcpy(g.R, rotation, sizeof(g.R));
  if (flags & GEO_SCALE) memcpy(g.s, scale, sizeof(g.s));
  g.snorm = scale_norm;
  g.axis = flip_axis;
  const int vec = (dense16(x, ld_x, w) ? VEC_IN : 0) | (dense16(out, ld_out, w) ? VEC_OUT : 0);
  const int grid = stream_grid((n + 3) >> 2, THREADS);
  if (mode == GEO_POS)
    geometry_kernel<3, GEO_POS><<<grid, THREADS, 0, stream>>>(x, out, n, ld_x, ld_out, vec, flags,
                                                              seed_jitter, q, g);
  else if (mode == GEO_NORMAL)
    geometry_kernel<3, GEO_NORMAL><<<grid, THREADS, 0, stream>>>(x, out, n, ld_x, ld_out, vec,
                                                                 flags, seed_jitter, q, g);
  else
    geometry_kernel<7, GEO_EDGE7><<<grid, THREADS, 0, stream>>>(x, out, n, ld_x, ld_out, vec,
                                                                flags, seed_jitter, q, g);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_augment_color_range_f32(const float* color, int64_t n, int64_t ld, int jitter,
                                           uint64_t seed, double sigma, double trunc, double lo,
                                           double hi, float* range6, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 40) && ld >= 3, "bad shape");
  Noise q{};
  SPT_CHECK_ARG(!jitter || make_noise(sigma, trunc, lo, hi, &q),
                "jitter needs sigma > 0 and -1 <= lo < hi <= 1");
  if (n == 0) return 0;
  SPT_CHECK_ARG(color && range6, "null pointer");
  SPT_CHECK_ARG((((uintptr_t)color | (uintptr_t)range6) & 3) == 0, "misaligned pointer");
  if (hipMemsetD32Async((hipDeviceptr_t)range6, 0x7F800000, 3, stream) != hipSuccess ||
      hipMemsetD32Async((hipDeviceptr_t)(range6 + 3), (int)0xFF800000u, 3, stream) != hipSuccess)
    return fail(-2, "%s: hipMemsetD32Async failed", __func__);
  const int vec = dense16(color, ld, 3) ? VEC_IN : 0;
  int grid = stream_grid((n + 3) >> 2, THREADS);
  if (grid > 1024) grid = 1024;          // 6 atomics per workgroup on 6 addresses
  color_range_kernel<<<grid, THREADS, 0, stream>>>(color, n, ld, vec, jitter ? 1 : 0, seed, q,
                                                   range6);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_augment_color_f32(const float* color, float* out, int64_t n, int64_t ld_color,
                                     int64_t ld_out, int flags, uint64_t seed, double sigma,
                                     double trunc, double lo, double hi, const float* range6,
                                     float blend, float one_minus_blend, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 40) && ld_color >= 3 && ld_out >= 3, "bad shape");
  SPT_CHECK_ARG(flags >= 1 && flags <= COL_ALL, "flags must be a non-empty subset of 1|2|4");
  Noise q{};
  SPT_CHECK_ARG(!(flags & COL_JITTER) || make_noise(sigma, trunc, lo, hi, &q),
                "jitter needs sigma > 0 and -1 <= lo < hi <= 1");
  if (n == 0) return 0;
  SPT_CHECK_ARG(color && out, "null pointer");
  SPT_CHECK_ARG(!(flags & COL_CONTRAST) || range6, "auto-contrast needs the range record");
  SPT_CHECK_ARG((((uintptr_t)color | (uintptr_t)out | (uintptr_t)range6) & 3) == 0,
                "misaligned pointer");
  const int vec = (dense16(color, ld_color, 3) ? VEC_IN : 0) | (dense16(out, ld_out, 3) ? VEC_OUT : 0);
  const int grid = stream_grid((n + 3) >> 2, THREADS);
  color_kernel<<<grid, THREADS, 0, stream>>>(color, out, n, ld_color, ld_out, vec, flags, seed, q,
                                             range6, blend, one_minus_blend);
  SPT_CHECK_LAUNCH();
  return 0;
}
