// PointFeatures: the colour keys (rgb as [0, 1] floats, hsv, lab) and the local density.
//
// Replaces the radiometric half and the density of the reference's transform:
//
//   PointFeatures._process        src/transforms/point.py:116-182
//   to_float_rgb                  src/utils/color.py:17-22
//   rgb2hsv, rgb2lab              src/utils/features.py:8-86
//
// The reference converts with a dozen [N, 3] temporaries, boolean-mask assignments (each a
// nonzero, hence a host sync on a device tensor), two 3x3 matmuls and a host read of rgb.max();
// the density takes three passes over the [N, k] tables.  Here:
//
//   color_flag_kernel   one read of rgb: "some value > 1" (and "some NaN") left in device memory
//   color_kernel        one read of rgb, any subset of {rgb, hsv, lab} written through
//                       (pointer, row stride): into tensors of their own or into a column block
//                       of a wider [N, F] table.  A lane owns 4 consecutive points: 12 bytes of
//                       uint8 are three dwords, a dense [N, 3] output three 16-byte stores; the
//                       last N % 4 points, strided outputs and unaligned bases take per-point
//                       loads / stores of the SAME values.
//   density_kernel      k_n / dmax_n^2 from the two kNN tables read in place (leading dimension)
//
// Arithmetic: the reference's f32 operations in the reference's order, IEEE division (never a
// reciprocal multiply), accurate powf / cbrtf, no contraction (-ffp-contract=off).  The only
// liberties: cbrtf(t) for t ** (1 / 3.) and the 3x3 products summed left to right.  For uint8
// input the 256 linearised sRGB values are computed once per workgroup into LDS by the very
// function the float path calls per value, so both give the same bits.
#include <math.h>

#include "common.hpp"

namespace spt {
namespace pfeat {

constexpr int THREADS = 256;
enum { KEY_RGB = 1, KEY_HSV = 2, KEY_LAB = 4, KEY_ALL = 7 };
enum { VEC_IN = 8 };                       // vec word: bits 0..2 = dense aligned output per key
enum { FLAG_GT1 = 1, FLAG_NAN = 2 };

struct Out {
  float* p;        // first element of column 0 of the block (column offset applied)
  int64_t ld;      // floats between consecutive rows
};

// to_float_rgb (color.py:17-22): / 255 when the global max is > 1, clamp to [0, 1] (NaN kept)
__device__ __forceinline__ float unit(float c, bool div) {
  if (div) c = c / 255.0f;
  return c < 0.0f ? 0.0f : (c > 1.0f ? 1.0f : c);
}

// features.py:54-57
__device__ __forceinline__ float linear100(float c) {
  const float l = c > 0.04045f ? powf((c + 0.055f) / 1.055f, 2.4f) : c / 12.92f;
  return l * 100.0f;
}

// Tensor.round(decimals=4)
__device__ __forceinline__ float round4(float x) { return rintf(x * 1e4f) / 1e4f; }

// features.py:72-74
__device__ __forceinline__ float lab_f(float t) {
  return t > 0.008856f ? cbrtf(t) : 7.787f * t + (float)(1.0 / 7.25);
}

// rgb2hsv (features.py:22-37) and the / 360 of point.py:141
__device__ __forceinline__ void hsv_of(float r, float g, float b, float* o) {
  const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b);
  const float mm = (mx - mn) + 1e-10f;
  const float h1 = 60.0f * (g - r) / mm + 60.0f;
  const float h2 = 60.0f * (b - g) / mm + 180.0f;
  const float h3 = 60.0f * (r - b) / mm + 300.0f;
  // (h2, h3, h1)[argmin], the first minimal channel on ties
  const float h = (r <= g && r <= b) ? h2 : (g <= b ? h3 : h1);
  o[0] = h / 360.0f;
  o[1] = mm / (mx + 1e-10f);
  o[2] = mx;
}

// rgb2lab after the linearisation (features.py:59-84) and the / 100 of point.py:150
__device__ __forceinline__ void lab_of(float r, float g, float b, float* o) {
  float x = round4((r * 0.4124f + g * 0.3576f) + b * 0.1805f);
  float y = round4((r * 0.2126f + g * 0.7152f) + b * 0.0722f);
  float z = round4((r * 0.0193f + g * 0.1192f) + b * 0.9505f);
  x = lab_f(x / 95.047f);
  y = lab_f(y / 100.0f);
  z = lab_f(z / 108.883f);
  const float L = 116.0f * y - 16.0f;
  const float A = 500.0f * x + -500.0f * y;
  const float B = 200.0f * y + -200.0f * z;
  o[0] = round4(L) / 100.0f;
  o[1] = round4(A) / 100.0f;
  o[2] = round4(B) / 100.0f;
}

// ---- "some value > 1" -------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void color_flag_u8_kernel(const uint8_t* __restrict__ rgb,
                                                               int64_t count, int aligned,
                                                               int* __restrict__ flag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool gt = false;
  const int64_t words = aligned ? count >> 2 : 0;
  const uint32_t* w = (const uint32_t*)rgb;
  for (int64_t i = tid; i < words; i += stride) gt |= (w[i] & 0xFEFEFEFEu) != 0u;
  for (int64_t i = words * 4 + tid; i < count; i += stride) gt |= rgb[i] > 1;
  if (__ballot(gt) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, FLAG_GT1);
}

__global__ __launch_bounds__(THREADS) void color_flag_f32_kernel(const float* __restrict__ rgb,
                                                                int64_t count,
                                                                int* __restrict__ flag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  bool gt = false, nan = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const float v = rgb[i];
    gt |= v > 1.0f;
    nan |= v != v;
  }
  const int f = (__ballot(gt) != 0ull ? FLAG_GT1 : 0) | (__ballot(nan) != 0ull ? FLAG_NAN : 0);
  if (f && (threadIdx.x & 63) == 0) atomicOr(flag, f);
}

// ---- the colour keys --------------------------------------------------------------------------
__device__ __forceinline__ void store4(const Out& o, bool vec, int64_t i0, int np,
                                       const float* v) {
  if (vec && np == 4) {
    float4* q = (float4*)(o.p + i0 * 3);
    q[0] = make_float4(v[0], v[1], v[2], v[3]);
    q[1] = make_float4(v[4], v[5], v[6], v[7]);
    q[2] = make_float4(v[8], v[9], v[10], v[11]);
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (p < np) {
        float* q = o.p + (i0 + p) * o.ld;
        q[0] = v[p * 3];
        q[1] = v[p * 3 + 1];
        q[2] = v[p * 3 + 2];
      }
  }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void color_kernel(const T* __restrict__ rgb, int64_t n,
                                                        int mask, int vec,
                                                        const int* __restrict__ flag, Out o_rgb,
                                                        Out o_hsv, Out o_lab) {
  constexpr bool U8 = sizeof(T) == 1;
  __shared__ float lin_tab[256];
  // rgb.max() > 1 is False when the max is NaN
  const bool div = flag[0] == FLAG_GT1;
  if (U8 && (mask & KEY_LAB)) {
    lin_tab[threadIdx.x] = linear100(unit((float)threadIdx.x, div));
    __syncthreads();
  }
  const int64_t groups = (n + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
    const int64_t i0 = g * 4;
    const int np = (n - i0) < 4 ? (int)(n - i0) : 4;
    T raw[12];
    if ((vec & VEC_IN) && np == 4) {
      if constexpr (U8) {
        const uint32_t* q = (const uint32_t*)(rgb + i0 * 3);
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          raw[j] = (T)((w0 >> (8 * j)) & 0xFFu);
          raw[4 + j] = (T)((w1 >> (8 * j)) & 0xFFu);
          raw[8 + j] = (T)((w2 >> (8 * j)) & 0xFFu);
        }
      } else {
        const float4* q = (const float4*)(rgb + i0 * 3);
        const float4 a = q[0], b = q[1], c = q[2];
        raw[0] = a.x; raw[1] = a.y; raw[2] = a.z; raw[3] = a.w;
        raw[4] = b.x; raw[5] = b.y; raw[6] = b.z; raw[7] = b.w;
        raw[8] = c.x; raw[9] = c.y; raw[10] = c.z; raw[11] = c.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 12; ++j) raw[j] = j < np * 3 ? rgb[i0 * 3 + j] : (T)0;
    }
    float c[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) c[j] = unit((float)raw[j], div);
    if (mask & KEY_RGB) store4(o_rgb, vec & KEY_RGB, i0, np, c);
    if (mask & KEY_HSV) {
      float v[12];
#pragma unroll
      for (int p = 0; p < 4; ++p) hsv_of(c[p * 3], c[p * 3 + 1], c[p * 3 + 2], v + p * 3);
      store4(o_hsv, vec & KEY_HSV, i0, np, v);
    }
    if (mask & KEY_LAB) {
      float l[12], v[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        if constexpr (U8) l[j] = lin_tab[raw[j]];
        else l[j] = linear100(c[j]);
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) lab_of(l[p * 3], l[p * 3 + 1], l[p * 3 + 2], v + p * 3);
      store4(o_lab, vec & KEY_LAB, i0, np, v);
    }
  }
}

// ---- density ----------------------------------------------------------------------------------
// A wave owns `rows` consecutive rows: consecutive lanes read consecutive elements of the
// flattened [rows, k] block (coalesced also for k far from 64), the distances go to LDS with an
// odd row pitch, the validity of the indices as one ballot word per 64 elements; lane r then
// reduces row r from LDS and the wave writes `rows` consecutive results.
constexpr int DENS_WAVES = THREADS / 64;
constexpr int DENS_FLOATS = 3072;                   // per wave: 64 rows up to k = 47
constexpr int DENS_WORDS = DENS_FLOATS / 64 + 1;

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(THREADS) void density_kernel(const int64_t* __restrict__ nn,
                                                          int64_t ld_nn,
                                                          const float* __restrict__ dist,
                                                          int64_t ld_dist, int64_t n, int k,
                                                          int rows, int64_t chunks,
                                                          float* __restrict__ density) {
  __shared__ float d_lds[DENS_WAVES][DENS_FLOATS];
  __shared__ uint64_t m_lds[DENS_WAVES][DENS_WORDS];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float* dl = d_lds[wid];
  uint64_t* ml = m_lds[wid];
  const int kp = k | 1;                              // odd pitch: lanes reading rows hit 64 banks
  const int q = 64 / k, rem = 64 % k;                // row / column advance of 64 elements
  const int64_t wave = (int64_t)blockIdx.x * DENS_WAVES + wid;
  const int64_t nwaves = (int64_t)gridDim.x * DENS_WAVES;
  for (int64_t ch = wave; ch < chunks; ch += nwaves) {
    const int64_t row0 = ch * rows;
    const int nr = (n - row0) < rows ? (int)(n - row0) : rows;
    const int total = nr * k;                        // <= DENS_FLOATS
    const int steps = (total + 63) >> 6;
    int row = lane / k, col = lane % k;
    for (int t = 0; t < steps; ++t) {
      const bool ok = t * 64 + lane < total;
      float d = 0.0f;
      int64_t j = -1;
      if (ok) {
        d = dist[(row0 + row) * ld_dist + col];
        j = nn[(row0 + row) * ld_nn + col];
        dl[row * kp + col] = d;
      }
      const uint64_t valid = __ballot(ok && j >= 0);
      if (lane == 0) ml[t] = valid;
      row += q;
      col += rem;
      if (col >= k) { col -= k; ++row; }
    }
    wave_lds_sync();
    if (lane < nr) {
      float m = dl[lane * kp];
      for (int c = 1; c < k; ++c) {
        const float v = dl[lane * kp + c];
        m = (v > m || v != v) ? v : m;               // Tensor.max: NaN wins
      }
      const int lo = lane * k, hi = lo + k;
      int cnt = 0;
      for (int w = lo >> 6; w <= (hi - 1) >> 6; ++w) {
        uint64_t bits = ml[w];
        if (w == lo >> 6) bits &= ~0ull << (lo & 63);
        const int top = hi - w * 64;                 // bits of this word below hi
        if (top < 64) bits &= (1ull << top) - 1ull;
        cnt += __popcll(bits);
      }
      density[row0 + lane] = (float)cnt / (m * m);
    }
    wave_lds_sync();
  }
}

static inline int density_rows(int k) {
  const int r = DENS_FLOATS / (k | 1);
  return r > 64 ? 64 : r;
}

}  // namespace pfeat
}  // namespace spt

using namespace spt;
using namespace spt::pfeat;

extern "C" size_t spt_point_color_workspace_bytes(int64_t num_points) {
  (void)num_points;
  return 256;
}

extern "C" int spt_point_color_f32(const void* rgb, int rgb_is_u8, int64_t n, int keys,
                                   float* out_rgb, int64_t ld_rgb, float* out_hsv,
                                   int64_t ld_hsv, float* out_lab, int64_t ld_lab, void* ws,
                                   size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 40), "bad shape");
  SPT_CHECK_ARG(keys >= 1 && keys <= KEY_ALL, "keys must be a non-empty subset of rgb|hsv|lab");
  SPT_CHECK_ARG(!(keys & KEY_RGB) || ld_rgb >= 3, "row stride of rgb below 3");
  SPT_CHECK_ARG(!(keys & KEY_HSV) || ld_hsv >= 3, "row stride of hsv below 3");
  SPT_CHECK_ARG(!(keys & KEY_LAB) || ld_lab >= 3, "row stride of lab below 3");
  if (n == 0) return 0;
  SPT_CHECK_ARG(rgb && ws, "null pointer");
  SPT_CHECK_ARG((!(keys & KEY_RGB) || out_rgb) && (!(keys & KEY_HSV) || out_hsv) &&
                    (!(keys & KEY_LAB) || out_lab),
                "null pointer");
  SPT_CHECK_ARG(ws_bytes >= spt_point_color_workspace_bytes(n) && ((uintptr_t)ws & 3) == 0,
                "workspace too small or misaligned");
  int* flag = (int*)ws;
  if (hipMemsetAsync(flag, 0, sizeof(int), stream) != hipSuccess)
    return fail(-2, "%s: hipMemsetAsync failed", __func__);
  const int64_t count = n * 3;
  auto dense = [](const float* p, int64_t ld) { return ld == 3 && ((uintptr_t)p & 15) == 0; };
  int vec = 0;
  if ((keys & KEY_RGB) && dense(out_rgb, ld_rgb)) vec |= KEY_RGB;
  if ((keys & KEY_HSV) && dense(out_hsv, ld_hsv)) vec |= KEY_HSV;
  if ((keys & KEY_LAB) && dense(out_lab, ld_lab)) vec |= KEY_LAB;
  const Out o_rgb{out_rgb, ld_rgb}, o_hsv{out_hsv, ld_hsv}, o_lab{out_lab, ld_lab};
  const int grid = stream_grid((n + 3) >> 2, THREADS);
  if (rgb_is_u8) {
    const int aligned = ((uintptr_t)rgb & 3) == 0;
    if (aligned) vec |= VEC_IN;
    color_flag_u8_kernel<<<stream_grid(count >> 2, THREADS), THREADS, 0, stream>>>(
        (const uint8_t*)rgb, count, aligned, flag);
    SPT_CHECK_LAUNCH();
    color_kernel<uint8_t><<<grid, THREADS, 0, stream>>>((const uint8_t*)rgb, n, keys, vec, flag,
                                                        o_rgb, o_hsv, o_lab);
  } else {
    SPT_CHECK_ARG(((uintptr_t)rgb & 3) == 0, "misaligned float rgb");
    if (((uintptr_t)rgb & 15) == 0) vec |= VEC_IN;
    color_flag_f32_kernel<<<stream_grid(count, THREADS), THREADS, 0, stream>>>(
        (const float*)rgb, count, flag);
    SPT_CHECK_LAUNCH();
    color_kernel<float><<<grid, THREADS, 0, stream>>>((const float*)rgb, n, keys, vec, flag,
                                                      o_rgb, o_hsv, o_lab);
  }
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_point_density_f32(const int64_t* neighbor_index, int64_t ld_index,
                                     const float* neighbor_distance, int64_t ld_distance,
                                     int64_t n, int k, float* density, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(n >= 0 && k >= 1 && k <= 255, "bad shape (k must be in 1..255)");
  SPT_CHECK_ARG(ld_index >= k && ld_distance >= k, "leading dimension below k");
  if (n == 0) return 0;
  SPT_CHECK_ARG(neighbor_index && neighbor_distance && density, "null pointer");
  const int rows = density_rows(k);
  const int64_t chunks = ceil_div(n, rows);
  const int grid = stream_grid(chunks, DENS_WAVES);
  density_kernel<<<grid, THREADS, 0, stream>>>(neighbor_index, ld_index, neighbor_distance,
                                               ld_distance, n, k, rows, chunks, density);
  SPT_CHECK_LAUNCH();
  return 0;
}
