// GroundElevation: ground filters, RANSAC plane, elevation.
//
// Replaces the step of the preprocessing chain between the point features and the adjacency
// graph:
//
//   GroundElevation._process                 src/transforms/point.py:268-326
//   filter_by_z_distance_of_global_min       src/utils/ground.py:25-42
//   filter_by_local_z_min / xy_partition     src/utils/ground.py:45-71, src/utils/partition.py:17-50
//   filter_by_verticality                    src/utils/ground.py:74-97
//   single_plane_model (CPU branch)          src/utils/ground.py:116-131
//
// The reference bins the points with a sort (consecutive_cluster), takes a scatter_min, gathers
// the trimmed cloud with a boolean mask and leaves torch for the RANSAC fit.  Here:
//
//   spt_ground_bounds_f32     one read of pos: min z and the extent of the XY cell coordinates
//   spt_ground_cell_min_f32   one read of pos: lowest point of every cell of a DENSE cell table,
//                             64-bit integer atomic min on (order-preserving bits of z, index)
//   spt_ground_trim_f32       the filters as a bitmap of the points, scan, indices of the trimmed
//                             points in increasing point order, their number left on the device
//   spt_ground_ransac_f32     H hypotheses scored in one pass over the trimmed points (ballot +
//                             popcount, integer adds), best one, f64 refit on its inliers
//   spt_ground_elevation_f32  (z - (a x + b y + c)) / scale for every point
//
// Cell coordinate: trunc(x / grid) with an IEEE f32 division, what
// pos[:, 0].div(grid, rounding_mode='trunc') computes - NOT a floor and NOT a multiplication by
// 1 / grid: the two cells around the origin merge into one of twice the width.  (torch's device
// kernel for a Python-number divisor does multiply by an f32 1 / grid and so differs from torch
// on the CPU for points on cell boundaries; the CPU result is the one reproduced here.)
//
// Ties.  Among the points of a cell that share the lowest z the one with the lowest index wins
// (torch_scatter's argmin leaves it open); -0.0 and +0.0 are the same height.  Among hypotheses
// with the same inlier count the lowest hypothesis index wins.  Both rules are order-free, the
// moments are summed per workgroup and then in a fixed order: every output is bitwise
// reproducible.
//
// Requires n < 2^31.  A point whose z is NaN never wins a cell and never passes the z filter.
#include "radix_sort.hpp"

namespace spt {
namespace ground {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_H = 256;                 // hypotheses per call: planes and counters live in LDS
constexpr int MAX_REDUCE_BLOCKS = 512;     // workgroups of the scoring / moment passes
constexpr int NMOM = 10;                   // n, Sx, Sy, Sz, Sxx, Sxy, Syy, Sxz, Syz, (spare)
constexpr uint64_t EMPTY = ~0ull;

// status record (device doubles)
enum { ST_M = 0, ST_BEST_COUNT = 1, ST_BEST = 2, ST_A = 3, ST_B = 4, ST_C = 5, ST_VALID = 6,
       ST_REFIT = 7, ST_LEN = 8 };

struct Plane {
  double a, b, c;
};

// f32 -> u32 with the order of the floats (NaN with a clear sign bit above +inf)
__device__ __forceinline__ uint32_t ordered_bits(float z) {
  const uint32_t u = __float_as_uint(z + 0.0f);               // -0.0 -> +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// trunc(v / grid), IEEE division (partition.py:35-36)
__device__ __forceinline__ float cell_coord(float v, float grid) { return truncf(v / grid); }

// vertical residual of a point to a plane, f64 throughout (no contraction: -ffp-contract=off)
__device__ __forceinline__ double residual(const Plane& p, double x, double y, double z) {
  return fabs(z - ((p.a * x + p.b * y) + p.c));
}

// ---- bounds ----------------------------------------------------------------------------------
struct Bounds {
  float zmin, imin, imax, jmin, jmax;
};

__device__ __forceinline__ Bounds merge(Bounds a, const Bounds& b) {
  a.zmin = fminf(a.zmin, b.zmin);
  a.imin = fminf(a.imin, b.imin); a.imax = fmaxf(a.imax, b.imax);
  a.jmin = fminf(a.jmin, b.jmin); a.jmax = fmaxf(a.jmax, b.jmax);
  return a;
}

__device__ __forceinline__ Bounds block_merge(Bounds v, Bounds* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Bounds t;
    t.zmin = __shfl_xor(v.zmin, o, 64);
    t.imin = __shfl_xor(v.imin, o, 64); t.imax = __shfl_xor(v.imax, o, 64);
    t.jmin = __shfl_xor(v.jmin, o, 64); t.jmax = __shfl_xor(v.jmax, o, 64);
    v = merge(v, t);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  Bounds r = sh[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) r = merge(r, sh[w]);
  return r;
}

__device__ __forceinline__ Bounds no_bounds() {
  const float inf = __builtin_huge_valf();
  return Bounds{inf, inf, -inf, inf, -inf};
}

__global__ __launch_bounds__(THREADS) void bounds_kernel(const float* __restrict__ pos, int64_t n,
                                                         float grid, Bounds* __restrict__ part) {
  __shared__ Bounds sh[WAVES];
  Bounds v = no_bounds();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float x = pos[i * 3 + 0], y = pos[i * 3 + 1], z = pos[i * 3 + 2];
    Bounds p;
    p.zmin = z;
    p.imin = p.imax = grid > 0.f ? cell_coord(x, grid) : 0.f;
    p.jmin = p.jmax = grid > 0.f ? cell_coord(y, grid) : 0.f;
    v = merge(v, p);
  }
  v = block_merge(v, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

__global__ __launch_bounds__(THREADS) void bounds_finish_kernel(const Bounds* __restrict__ part,
                                                                int nblocks,
                                                                float* __restrict__ out) {
  __shared__ Bounds sh[WAVES];
  Bounds v = no_bounds();
  for (int b = threadIdx.x; b < nblocks; b += THREADS) v = merge(v, part[b]);
  v = block_merge(v, sh);
  if (threadIdx.x == 0) {
    out[0] = v.zmin; out[1] = v.imin; out[2] = v.imax; out[3] = v.jmin; out[4] = v.jmax;
  }
}

// ---- lowest point per cell -------------------------------------------------------------------
// The minimum only decreases: a load of the cell before the atomic skips every point that
// cannot win.  The load is a relaxed device-scope one (served by L2, never by the CU's L1); a
// stale value lets a few extra atomics through and never drops a winner.
__global__ __launch_bounds__(THREADS) void cell_min_kernel(
    const float* __restrict__ pos, int64_t n, float grid, double i_min, double j_min, int64_t ni,
    int64_t nj, uint64_t* __restrict__ table) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float x = pos[i * 3 + 0], y = pos[i * 3 + 1], z = pos[i * 3 + 2];
    const double ci = (double)cell_coord(x, grid) - i_min;
    const double cj = (double)cell_coord(y, grid) - j_min;
    if (!(ci >= 0.0 && ci < (double)ni && cj >= 0.0 && cj < (double)nj)) continue;   // NaN too
    if (z != z) continue;
    const int64_t cell = (int64_t)ci * nj + (int64_t)cj;
    const uint64_t key = ((uint64_t)ordered_bits(z) << 32) | (uint64_t)(uint32_t)i;
    unsigned long long* slot = (unsigned long long*)(table + cell);
    const uint64_t seen = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (key < seen) atomicMin(slot, (unsigned long long)key);
  }
}

// ---- filters -> bitmap of the points ---------------------------------------------------------
struct Filters {
  const float* pos;
  int64_t n;
  const float* bounds;         // bounds[0] = min z (device)
  int use_z;
  float z_threshold;
  const float* verticality;    // nullable
  float v_threshold;
};

__device__ __forceinline__ bool passes(const Filters& f, int64_t i) {
  bool ok = true;
  if (f.use_z) ok = ok && (f.pos[i * 3 + 2] - f.bounds[0] < f.z_threshold);   // ground.py:42
  if (f.verticality) ok = ok && (f.verticality[i] < f.v_threshold);          // ground.py:97
  return ok;
}

// one 64-bit ballot per wave and 64 points: every word of the bitmap is written, no atomics
__global__ __launch_bounds__(THREADS) void point_mask_kernel(Filters f, int64_t num_words,
                                                             uint32_t* __restrict__ words) {
  const int64_t wave = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * WAVES;
  const int lane = threadIdx.x & 63;
  for (int64_t base = wave * 64; base < f.n; base += nwaves * 64) {
    const int64_t i = base + lane;
    const bool ok = i < f.n && passes(f, i);
    const uint64_t ballot = __ballot(ok);
    if (lane == 0) {
      const int64_t w = base >> 5;
      words[w] = (uint32_t)ballot;
      if (w + 1 < num_words) words[w + 1] = (uint32_t)(ballot >> 32);
    }
  }
}

// the winners of the cell table that pass the other filters set their bit (bitmap cleared before)
__global__ __launch_bounds__(THREADS) void cell_mask_kernel(Filters f,
                                                            const uint64_t* __restrict__ table,
                                                            int64_t num_cells,
                                                            uint32_t* __restrict__ words) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < num_cells; c += stride) {
    const uint64_t key = table[c];
    if (key == EMPTY) continue;
    const int64_t i = (int64_t)(uint32_t)key;
    if (i >= f.n || !passes(f, i)) continue;
    atomicOr(&words[i >> 5], 1u << (i & 31));
  }
}

// offs[w] = popcount(words[w]), offs[num_words] = 0 (becomes the total under the scan)
__global__ __launch_bounds__(THREADS) void popcount_kernel(const uint32_t* __restrict__ words,
                                                           int64_t num_words,
                                                           uint32_t* __restrict__ offs) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= num_words; w += stride)
    offs[w] = w < num_words ? (uint32_t)__popc(words[w]) : 0u;
}

__global__ __launch_bounds__(THREADS) void emit_kernel(const uint32_t* __restrict__ words,
                                                       const uint32_t* __restrict__ offs,
                                                       int64_t num_words, int64_t capacity,
                                                       int64_t* __restrict__ index,
                                                       int64_t* __restrict__ count) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < num_words; w += stride) {
    uint32_t bits = words[w];
    int64_t at = offs[w];
    while (bits) {
      const int b = __ffs((int)bits) - 1;
      bits &= bits - 1;
      if (at < capacity) index[at] = w * 32 + b;
      ++at;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t m = offs[num_words];
    *count = m < capacity ? m : capacity;
  }
}

// ---- RANSAC ----------------------------------------------------------------------------------
__device__ __forceinline__ int64_t trimmed_count(const int64_t* count, int64_t capacity) {
  const int64_t m = *count;
  return m < 0 ? 0 : (m < capacity ? m : capacity);
}

// hypothesis h: three trimmed points -> plane z = a x + b y + c through them; NaN plane and
// valid[h] = 0 for a repeated / out-of-range index or a triangle that is degenerate in XY
// (|sin| of the angle between two of its edges <= 1e-9)
__global__ __launch_bounds__(MAX_H) void hypotheses_kernel(
    const float* __restrict__ pos, int64_t n, const int64_t* __restrict__ index,
    const int64_t* __restrict__ count, int64_t capacity, const float* __restrict__ u,
    const int64_t* __restrict__ samples, int H, Plane* __restrict__ planes,
    int32_t* __restrict__ valid) {
  const int h = threadIdx.x;
  if (h >= H) return;
  const int64_t M = trimmed_count(count, capacity);
  const double nan = __builtin_nan("");
  Plane pl{nan, nan, nan};
  int ok = 1;
  int64_t s[3];
  for (int q = 0; q < 3; ++q) {
    if (samples) {
      s[q] = samples[h * 3 + q];
    } else {
      const double t = floor((double)u[h * 3 + q] * (double)M);
      s[q] = t >= (double)M ? M - 1 : (int64_t)t;          // min(floor(u M), M - 1)
    }
    if (s[q] < 0 || s[q] >= M) ok = 0;
  }
  if (ok && (s[0] == s[1] || s[0] == s[2] || s[1] == s[2])) ok = 0;
  double p[3][3];
  if (ok) {
    for (int q = 0; q < 3; ++q) {
      const int64_t i = index[s[q]];
      if (i < 0 || i >= n) { ok = 0; break; }
      for (int d = 0; d < 3; ++d) p[q][d] = (double)pos[i * 3 + d];
    }
  }
  if (ok) {
    const double dx1 = p[1][0] - p[0][0], dy1 = p[1][1] - p[0][1], dz1 = p[1][2] - p[0][2];
    const double dx2 = p[2][0] - p[0][0], dy2 = p[2][1] - p[0][1], dz2 = p[2][2] - p[0][2];
    const double det = dx1 * dy2 - dx2 * dy1;
    const double n1 = dx1 * dx1 + dy1 * dy1, n2 = dx2 * dx2 + dy2 * dy2;
    if (!(det * det > 1e-18 * (n1 * n2))) {
      ok = 0;
    } else {
      pl.a = (dz1 * dy2 - dz2 * dy1) / det;
      pl.b = (dx1 * dz2 - dx2 * dz1) / det;
      pl.c = p[0][2] - (pl.a * p[0][0] + pl.b * p[0][1]);
      if (!(pl.a == pl.a && pl.b == pl.b && pl.c == pl.c)) { ok = 0; pl = Plane{nan, nan, nan}; }
    }
  }
  planes[h] = pl;
  valid[h] = ok;
}

// All hypotheses against every trimmed point in one pass: the planes sit in LDS, each wave takes
// 64 points, one ballot + popcount per hypothesis, per-wave counters in LDS, then one integer
// atomic add per hypothesis and workgroup.
__global__ __launch_bounds__(THREADS) void score_kernel(
    const float* __restrict__ pos, int64_t n, const int64_t* __restrict__ index,
    const int64_t* __restrict__ count, int64_t capacity, const Plane* __restrict__ planes, int H,
    double threshold, int32_t* __restrict__ counts) {
  __shared__ Plane sh_plane[MAX_H];
  __shared__ uint32_t sh_cnt[WAVES][MAX_H];
  const int64_t M = trimmed_count(count, capacity);
  if ((int64_t)blockIdx.x * THREADS >= M) return;                 // nothing to add
  for (int h = threadIdx.x; h < H; h += THREADS) sh_plane[h] = planes[h];
  for (int h = threadIdx.x; h < WAVES * MAX_H; h += THREADS) (&sh_cnt[0][0])[h] = 0u;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t base = (int64_t)blockIdx.x * THREADS + wave * 64; base < M; base += stride) {
    const int64_t j = base + lane;
    bool live = j < M;
    double x = 0.0, y = 0.0, z = 0.0;
    if (live) {
      const int64_t i = index[j];
      live = i >= 0 && i < n;
      if (live) { x = (double)pos[i * 3 + 0]; y = (double)pos[i * 3 + 1]; z = (double)pos[i * 3 + 2]; }
    }
    for (int h = 0; h < H; ++h) {
      const bool in = live && residual(sh_plane[h], x, y, z) < threshold;
      const uint64_t ballot = __ballot(in);
      if (lane == 0) sh_cnt[wave][h] += (uint32_t)__popcll(ballot);
    }
  }
  __syncthreads();
  for (int h = threadIdx.x; h < H; h += THREADS) {
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) c += sh_cnt[w][h];
    if (c) atomicAdd(&counts[h], (int32_t)c);
  }
}

// counts[h] = -1 for the invalid hypotheses; best = largest count, lowest index among equals
__global__ __launch_bounds__(MAX_H) void select_kernel(const int64_t* __restrict__ count,
                                                       int64_t capacity,
                                                       const Plane* __restrict__ planes,
                                                       const int32_t* __restrict__ valid, int H,
                                                       int32_t* __restrict__ counts,
                                                       Plane* __restrict__ best_plane,
                                                       double* __restrict__ status) {
  __shared__ int32_t sh[MAX_H];
  const int h = threadIdx.x;
  if (h < H) {
    const int32_t c = valid[h] ? counts[h] : -1;
    counts[h] = c;
    sh[h] = c;
  }
  __syncthreads();
  if (h != 0) return;
  int best = -1, nvalid = 0;
  int32_t best_count = -1;
  for (int q = 0; q < H; ++q) {
    if (sh[q] < 0) continue;
    ++nvalid;
    if (sh[q] > best_count) { best_count = sh[q]; best = q; }
  }
  const double nan = __builtin_nan("");
  *best_plane = best >= 0 ? planes[best] : Plane{nan, nan, nan};
  status[ST_M] = (double)trimmed_count(count, capacity);
  status[ST_BEST_COUNT] = (double)best_count;
  status[ST_BEST] = (double)best;
  status[ST_VALID] = (double)nvalid;
}

// block sum in a fixed order: lanes by butterfly, then the waves in sequence
__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = wave_reduce_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// moments of the best hypothesis's inliers about `origin` = the first trimmed point (keeps the
// coordinates small whatever the cloud's offset), per-workgroup partials into a slab
__global__ __launch_bounds__(THREADS) void moments_kernel(
    const float* __restrict__ pos, int64_t n, const int64_t* __restrict__ index,
    const int64_t* __restrict__ count, int64_t capacity, const Plane* __restrict__ best_plane,
    double threshold, double* __restrict__ part) {
  __shared__ double sh[WAVES];
  const int64_t M = trimmed_count(count, capacity);
  const Plane pl = *best_plane;
  double ox = 0.0, oy = 0.0, oz = 0.0;
  if (M > 0) {
    const int64_t i0 = index[0];
    if (i0 >= 0 && i0 < n) { ox = (double)pos[i0 * 3 + 0]; oy = (double)pos[i0 * 3 + 1]; oz = (double)pos[i0 * 3 + 2]; }
  }
  double m[NMOM];
#pragma unroll
  for (int q = 0; q < NMOM; ++q) m[q] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t j = (int64_t)blockIdx.x * THREADS + threadIdx.x; j < M; j += stride) {
    const int64_t i = index[j];
    if (i < 0 || i >= n) continue;
    const double x = (double)pos[i * 3 + 0], y = (double)pos[i * 3 + 1], z = (double)pos[i * 3 + 2];
    if (!(residual(pl, x, y, z) < threshold)) continue;
    const double dx = x - ox, dy = y - oy, dz = z - oz;
    m[0] += 1.0; m[1] += dx; m[2] += dy; m[3] += dz;
    m[4] += dx * dx; m[5] += dx * dy; m[6] += dy * dy; m[7] += dx * dz; m[8] += dy * dz;
  }
#pragma unroll
  for (int q = 0; q < NMOM; ++q) {
    const double t = block_sum(m[q], sh);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * NMOM + q] = t;
  }
}

// the slab summed in a fixed order, the least-squares plane of the inliers (sklearn's final
// LinearRegression: centred normal equations), status[3..5] = (a, b, c).  A rank-deficient
// inlier set (fewer than 3 inliers, or all on one line in XY) keeps the hypothesis's own plane
// and reports status[7] = -1; otherwise status[7] = number of inliers used.
__global__ __launch_bounds__(THREADS) void solve_kernel(
    const float* __restrict__ pos, int64_t n, const int64_t* __restrict__ index,
    const int64_t* __restrict__ count, int64_t capacity, const Plane* __restrict__ best_plane,
    const double* __restrict__ part, int nblocks, double* __restrict__ status) {
  __shared__ double sh[WAVES];
  double m[NMOM];
  for (int q = 0; q < NMOM; ++q) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += THREADS) s += part[(int64_t)b * NMOM + q];
    m[q] = block_sum(s, sh);
  }
  if (threadIdx.x != 0) return;
  const int64_t M = trimmed_count(count, capacity);
  double ox = 0.0, oy = 0.0, oz = 0.0;
  if (M > 0) {
    const int64_t i0 = index[0];
    if (i0 >= 0 && i0 < n) { ox = (double)pos[i0 * 3 + 0]; oy = (double)pos[i0 * 3 + 1]; oz = (double)pos[i0 * 3 + 2]; }
  }
  Plane pl = *best_plane;
  double used = -1.0;
  const double cnt = m[0];
  if (cnt >= 3.0) {
    const double mx = m[1] / cnt, my = m[2] / cnt, mz = m[3] / cnt;
    const double cxx = m[4] - m[1] * mx, cxy = m[5] - m[1] * my, cyy = m[6] - m[2] * my;
    const double cxz = m[7] - m[1] * mz, cyz = m[8] - m[2] * mz;
    const double det = cxx * cyy - cxy * cxy;
    if (det > 1e-12 * (cxx * cyy) && cxx > 0.0 && cyy > 0.0) {
      const double a = (cxz * cyy - cyz * cxy) / det;
      const double b = (cyz * cxx - cxz * cxy) / det;
      pl.a = a;
      pl.b = b;
      pl.c = (mz + oz) - (a * (mx + ox) + b * (my + oy));
      used = cnt;
    }
  }
  status[ST_A] = pl.a; status[ST_B] = pl.b; status[ST_C] = pl.c;
  status[ST_REFIT] = used;
}

__global__ __launch_bounds__(THREADS) void elevation_kernel(const float* __restrict__ pos, int64_t n,
                                                            const double* __restrict__ status,
                                                            double scale,
                                                            float* __restrict__ elevation) {
  const Plane pl{status[ST_A], status[ST_B], status[ST_C]};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double x = (double)pos[i * 3 + 0], y = (double)pos[i * 3 + 1], z = (double)pos[i * 3 + 2];
    elevation[i] = (float)((z - ((pl.a * x + pl.b * y) + pl.c)) / scale);
  }
}

static int reduce_grid(int64_t n, int cap) {
  int64_t b = ceil_div(n > 0 ? n : 1, THREADS);
  if (b > cap) b = cap;
  return (int)b;
}

static bool count_ok(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31); }

struct TrimPlan {
  int64_t words;
  size_t off_words, off_offs, off_part, total;
  int64_t part_cap;
};

static TrimPlan trim_plan(int64_t n) {
  TrimPlan p;
  p.words = ceil_div(n > 0 ? n : 1, 32);
  size_t o = 0;
  p.off_words = o; o += align_up((size_t)(p.words + 1) * 4, 256);
  p.off_offs = o;  o += align_up((size_t)(p.words + 1) * 4, 256);
  p.off_part = o;  o += scan_part_bytes(p.words + 1);
  p.part_cap = (int64_t)((o - p.off_part) / 4);
  p.total = o;
  return p;
}

struct RansacPlan {
  size_t off_planes, off_best, off_valid, off_part, total;
};

static RansacPlan ransac_plan() {
  RansacPlan p;
  size_t o = 0;
  p.off_planes = o; o += align_up(sizeof(Plane) * MAX_H, 256);
  p.off_best = o;   o += align_up(sizeof(Plane), 256);
  p.off_valid = o;  o += align_up(sizeof(int32_t) * MAX_H, 256);
  p.off_part = o;   o += align_up(sizeof(double) * NMOM * MAX_REDUCE_BLOCKS, 256);
  p.total = o;
  return p;
}

}  // namespace ground
}  // namespace spt

using namespace spt;
using namespace spt::ground;

extern "C" size_t spt_ground_bounds_workspace_bytes(int64_t num_points) {
  if (num_points < 0) return 0;
  return align_up((size_t)reduce_grid(num_points, 1024) * sizeof(Bounds), 256);
}

extern "C" int spt_ground_bounds_f32(const float* pos, int64_t num_points, float grid,
                                     float* bounds, void* ws, size_t ws_bytes,
                                     spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t n = num_points;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "num_points out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(pos && bounds, "null pointer");
  SPT_CHECK_ARG(grid == grid, "grid is NaN");
  SPT_CHECK_ARG(ws && ws_bytes >= spt_ground_bounds_workspace_bytes(n), "workspace too small");
  const int g = reduce_grid(n, 1024);
  bounds_kernel<<<g, THREADS, 0, stream>>>(pos, n, grid, (Bounds*)ws);
  bounds_finish_kernel<<<1, THREADS, 0, stream>>>((const Bounds*)ws, g, bounds);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_ground_cell_min_f32(const float* pos, int64_t num_points, float grid,
                                       int64_t i_min, int64_t j_min, int64_t num_i, int64_t num_j,
                                       uint64_t* table, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t n = num_points;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "num_points out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(grid > 0.f, "grid must be positive");
  SPT_CHECK_ARG(num_i >= 1 && num_j >= 1 && num_i <= ((int64_t)1 << 31) &&
                    num_j <= ((int64_t)1 << 31) && num_i * num_j <= ((int64_t)1 << 31),
                "cell table out of range (at most 2^31 cells)");
  SPT_CHECK_ARG(pos && table, "null pointer");
  (void)hipMemsetAsync(table, 0xFF, (size_t)(num_i * num_j) * 8, stream);
  cell_min_kernel<<<stream_grid(n, THREADS), THREADS, 0, stream>>>(
      pos, n, grid, (double)i_min, (double)j_min, num_i, num_j, table);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_ground_trim_workspace_bytes(int64_t num_points) {
  if (num_points < 0) return 0;
  return trim_plan(num_points).total;
}

extern "C" int spt_ground_trim_f32(const float* pos, int64_t num_points, const float* bounds,
                                   int use_z, float z_threshold, const float* verticality,
                                   float verticality_threshold, const uint64_t* table,
                                   int64_t num_cells, int64_t* index, int64_t capacity,
                                   int64_t* count, void* ws, size_t ws_bytes,
                                   spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t n = num_points;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "num_points out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(pos && index && count, "null pointer");
  SPT_CHECK_ARG(!use_z || bounds, "the z filter needs the bounds");
  SPT_CHECK_ARG(capacity >= 1, "capacity must be positive");
  SPT_CHECK_ARG(!table || (num_cells >= 1 && num_cells <= ((int64_t)1 << 31)),
                "cell table out of range");
  const TrimPlan p = trim_plan(n);
  SPT_CHECK_ARG(ws && ws_bytes >= p.total, "workspace too small");
  uint32_t* words = (uint32_t*)((char*)ws + p.off_words);
  uint32_t* offs = (uint32_t*)((char*)ws + p.off_offs);
  uint32_t* part = (uint32_t*)((char*)ws + p.off_part);
  const Filters f{pos, n, bounds, use_z ? 1 : 0, z_threshold, verticality, verticality_threshold};
  if (table) {
    (void)hipMemsetAsync(words, 0, (size_t)p.words * 4, stream);
    cell_mask_kernel<<<stream_grid(num_cells, THREADS), THREADS, 0, stream>>>(f, table, num_cells,
                                                                              words);
  } else {
    point_mask_kernel<<<stream_grid(n, THREADS), THREADS, 0, stream>>>(f, p.words, words);
  }
  popcount_kernel<<<stream_grid(p.words + 1, THREADS), THREADS, 0, stream>>>(words, p.words, offs);
  SPT_CHECK_ARG(device_exclusive_scan(offs, p.words + 1, part, p.part_cap, stream) == 0,
                "scan partials do not fit their region");
  emit_kernel<<<stream_grid(p.words, THREADS), THREADS, 0, stream>>>(words, offs, p.words,
                                                                     capacity, index, count);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_ground_ransac_workspace_bytes(int num_hypotheses) {
  if (num_hypotheses < 1 || num_hypotheses > MAX_H) return 0;
  return ransac_plan().total;
}

extern "C" int spt_ground_ransac_f32(const float* pos, int64_t num_points, const int64_t* index,
                                     const int64_t* count, int64_t capacity, const float* u,
                                     const int64_t* samples, int num_hypotheses,
                                     double residual_threshold, int32_t* counts, double* status,
                                     void* ws, size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t n = num_points;
  const int H = num_hypotheses;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "num_points out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(H >= 1 && H <= MAX_H, "num_hypotheses out of range (1 .. 256)");
  SPT_CHECK_ARG(capacity >= 1 && count_ok(capacity), "capacity out of range");
  SPT_CHECK_ARG(pos && index && count && counts && status, "null pointer");
  SPT_CHECK_ARG((u != nullptr) != (samples != nullptr), "exactly one of u and samples");
  SPT_CHECK_ARG(residual_threshold == residual_threshold, "residual_threshold is NaN");
  const RansacPlan p = ransac_plan();
  SPT_CHECK_ARG(ws && ws_bytes >= p.total, "workspace too small");
  Plane* planes = (Plane*)((char*)ws + p.off_planes);
  Plane* best = (Plane*)((char*)ws + p.off_best);
  int32_t* valid = (int32_t*)((char*)ws + p.off_valid);
  double* part = (double*)((char*)ws + p.off_part);
  const int g = reduce_grid(capacity, MAX_REDUCE_BLOCKS);
  (void)hipMemsetAsync(counts, 0, (size_t)H * 4, stream);
  hypotheses_kernel<<<1, MAX_H, 0, stream>>>(pos, n, index, count, capacity, u, samples, H,
                                             planes, valid);
  score_kernel<<<g, THREADS, 0, stream>>>(pos, n, index, count, capacity, planes, H,
                                          residual_threshold, counts);
  select_kernel<<<1, MAX_H, 0, stream>>>(count, capacity, planes, valid, H, counts, best, status);
  moments_kernel<<<g, THREADS, 0, stream>>>(pos, n, index, count, capacity, best,
                                            residual_threshold, part);
  solve_kernel<<<1, THREADS, 0, stream>>>(pos, n, index, count, capacity, best, part, g, status);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_ground_elevation_f32(const float* pos, int64_t num_points, const double* status,
                                        float scale, float* elevation, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t n = num_points;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "num_points out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(pos && status && elevation, "null pointer");
  SPT_CHECK_ARG(scale > 0.f, "scale must be positive");
  elevation_kernel<<<stream_grid(n, THREADS), THREADS, 0, stream>>>(pos, n, status, (double)scale,
                                                                    elevation);
  SPT_CHECK_LAUNCH();
  return 0;
}
