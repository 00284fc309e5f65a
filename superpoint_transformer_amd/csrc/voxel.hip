// GridSampling3D on the device (src/transforms/sampling.py:86-468): integer voxel coordinates,
// a u64 key per point, ONE stable sort of (key, point), run heads -> groups, and the per-voxel
// reductions (mean, label histogram, vote, representative) over those groups.
//
// coordinate = rintf(pos / size): `/` is the correctly rounded IEEE division (no reciprocal, no
// fast-math flag on this file) and rintf rounds half to even - bit for bit torch.round(pos / size).
//
// No kernel uses a key, a coordinate or a label as an address: keys are only sorted and compared,
// labels are range-checked before they index a row.  Every index into an output is a sorted
// position (< n) or a voxel id (< V <= n).
#include "common.hpp"
#include "rng.hpp"
#include "sorted_runs.hpp"

#include <limits.h>

namespace spt {
namespace {

constexpr int THREADS = 256;
constexpr int LONG_RUN = 512;     // runs longer than this are reduced by a whole wave
constexpr int VOTE_SHORT = 16;    // vote: runs up to this are counted pairwise by one lane
constexpr int MAX_LABEL_BINS = 256;

inline bool count_ok(int64_t n) { return n >= 0 && n <= (int64_t)INT32_MAX; }

// record of spt_voxel_bounds_f32
enum { R_XMIN = 0, R_XMAX, R_YMIN, R_YMAX, R_ZMIN, R_ZMAX, R_BMIN, R_BMAX, R_NONFINITE, R_RANGE,
       R_LEN };

__global__ void bounds_init_kernel(int32_t* __restrict__ rec, int has_batch) {
  const int t = threadIdx.x;
  if (t < R_LEN) {
    int32_t v = 0;
    if (t < 6 || has_batch) {
      if (t == R_XMIN || t == R_YMIN || t == R_ZMIN || t == R_BMIN) v = INT32_MAX;
      if (t == R_XMAX || t == R_YMAX || t == R_ZMAX || t == R_BMAX) v = INT32_MIN;
    }
    if (t >= R_NONFINITE) v = 0;
    rec[t] = v;
  }
}

// 0 = usable, 1 = non-finite, 2 = outside the int32 range
__device__ __forceinline__ int voxel_coord(float p, float size, int32_t* c) {
  const float q = rintf(p / size);
  if (!(fabsf(q) <= 3.4028234663852886e38f)) return 1;   // NaN or inf
  if (!(fabsf(q) <= 2147483520.f)) return 2;             // largest f32 below 2^31
  *c = (int32_t)q;
  return 0;
}

__global__ __launch_bounds__(THREADS) void bounds_kernel(
    const float* __restrict__ pos, int64_t n, int64_t ld, float size,
    const int64_t* __restrict__ batch, int32_t* __restrict__ rec) {
  int32_t lo[4] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX};
  int32_t hi[4] = {INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN};
  int32_t nonfinite = 0, range = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int32_t c[4] = {0, 0, 0, 0};
    int bad = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) bad |= voxel_coord(pos[i * ld + a], size, &c[a]);
    if (batch) {
      const int64_t b = batch[i];
      if (b < -(int64_t)INT32_MAX || b > (int64_t)INT32_MAX) bad |= 2;
      else c[3] = (int32_t)b;
    }
    if (bad) {
      nonfinite += bad & 1;
      range += (bad & 1) ? 0 : 1;
      continue;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      lo[a] = min(lo[a], c[a]);
      hi[a] = max(hi[a], c[a]);
    }
  }
  // wave butterfly, then one set of atomics per workgroup through LDS
  __shared__ int32_t s[THREADS / 64][10];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      lo[a] = min(lo[a], __shfl_xor(lo[a], o, 64));
      hi[a] = max(hi[a], __shfl_xor(hi[a], o, 64));
    }
    nonfinite += __shfl_xor(nonfinite, o, 64);
    range += __shfl_xor(range, o, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      s[w][2 * a] = lo[a];
      s[w][2 * a + 1] = hi[a];
    }
    s[w][8] = nonfinite;
    s[w][9] = range;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < R_LEN) {
    if (t >= 6 && t < 8 && !batch) return;
    int32_t v = s[0][t];
    for (int k = 1; k < THREADS / 64; ++k) {
      const int32_t u = s[k][t];
      if (t >= R_NONFINITE) v += u;
      else if (t & 1) v = max(v, u);
      else v = min(v, u);
    }
    if (t >= R_NONFINITE) {
      if (v) atomicAdd(&rec[t], v);
    } else if (t & 1) {
      atomicMax(&rec[t], v);
    } else {
      atomicMin(&rec[t], v);
    }
  }
}

struct KeyLayout {
  int64_t origin[4];   // x, y, z, batch
  int bits[4];
};

// (batch, z, y, x) - origin, x in the low bits.  Fields are masked to their width, so a point
// the record did not cover (none, when the host checked the record) still yields a valid key.
__global__ __launch_bounds__(THREADS) void keys_kernel(
    const float* __restrict__ pos, int64_t n, int64_t ld, float size,
    const int64_t* __restrict__ batch, KeyLayout L, uint32_t* __restrict__ lo32,
    uint32_t* __restrict__ hi32) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int64_t c[4] = {0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int32_t v = 0;
      voxel_coord(pos[i * ld + a], size, &v);
      c[a] = v;
    }
    if (batch) c[3] = batch[i];
    uint64_t key = 0;
    int shift = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const uint64_t mask = L.bits[a] ? ((~0ull) >> (64 - L.bits[a])) : 0ull;
      key |= ((uint64_t)(c[a] - L.origin[a]) & mask) << shift;
      shift += L.bits[a];
    }
    lo32[i] = (uint32_t)key;
    if (hi32) hi32[i] = (uint32_t)(key >> 32);
  }
}

// excl: the scanned run flags of csrc/sorted_runs.hpp - excl[i + 1] - 1 is the voxel of sorted
// position i and excl[n] = V
__global__ void groups_kernel(SortedKeys keys, const uint32_t* __restrict__ excl, int64_t n,
                              KeyLayout L, int64_t* __restrict__ pointers,
                              int64_t* __restrict__ cluster, int64_t* __restrict__ order,
                              int64_t* __restrict__ last, int32_t* __restrict__ coords,
                              int64_t* __restrict__ count) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t before = excl[i], upto = excl[i + 1];       // heads in [0, i) and in [0, i]
    const int64_t v = (int64_t)upto - 1;                       // 0 <= v < V <= n
    const int64_t p = keys.order[i];
    order[i] = p;
    cluster[p] = v;
    if (upto != before) {                                      // a run starts here
      pointers[v] = i;
      const uint64_t key = sorted_key(keys, i);
      int shift = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const uint64_t mask = L.bits[a] ? ((~0ull) >> (64 - L.bits[a])) : 0ull;
        coords[v * 3 + a] = (int32_t)((int64_t)((key >> shift) & mask) + L.origin[a]);
        shift += L.bits[a];
      }
    }
    const bool ends = (i == n - 1) || excl[i + 2] != upto;     // (excl has n + 1 entries)
    if (ends) last[v] = p;
    if (i == n - 1) {
      pointers[v + 1] = n;
      *count = v + 1;
    }
  }
}

// ---- reductions over the groups ----------------------------------------------------------------
// One lane per (voxel, column): the lanes of a voxel read neighbouring floats of a row.  A long
// run is taken by the whole wave afterwards, one after the other.
__global__ __launch_bounds__(THREADS) void mean_kernel(
    const float* __restrict__ x, int cols, int64_t ld_x, const int64_t* __restrict__ pointers,
    const int64_t* __restrict__ order, int64_t num_voxels, float* __restrict__ out,
    int64_t ld_out) {
  const int lane = threadIdx.x & 63;
  const int64_t total = num_voxels * cols;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < total;
       base += stride) {                                      // wave-uniform trip count
    const int64_t t = base + lane;
    int64_t v = 0, b = 0, e = 0;
    int c = 0;
    if (t < total) {
      v = t / cols;
      c = (int)(t - v * cols);
      b = pointers[v];
      e = pointers[v + 1];
    }
    const bool longrun = e - b > LONG_RUN;
    if (t < total && !longrun) {
      float s = 0.0f;
      for (int64_t j = b; j < e; ++j) s += x[order[j] * ld_x + c];
      out[v * ld_out + c] = s / (float)(e - b);
    }
    uint64_t todo = __ballot(longrun);
    while (todo) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const int64_t b2 = __shfl(b, src, 64), e2 = __shfl(e, src, 64), v2 = __shfl(v, src, 64);
      const int c2 = __shfl(c, src, 64);
      float s = 0.0f;
      for (int64_t j = b2 + lane; j < e2; j += 64) s += x[order[j] * ld_x + c2];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);   // fixed tree
      if (lane == 0) out[v2 * ld_out + c2] = s / (float)(e2 - b2);
    }
  }
}

__global__ void normalize3_kernel(float* __restrict__ out, int64_t ld_out, int64_t num_voxels) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < num_voxels; v += stride) {
    float* r = out + v * ld_out;
    const float a = r[0], b = r[1], c = r[2];
    const float nrm = sqrtf(a * a + b * b + c * c);
    r[0] = a / nrm;
    r[1] = b / nrm;
    r[2] = c / nrm;
  }
}

// hist != null: one lane owns the [n_bins] row of its voxel.  vote != null (hist null): runs up
// to VOTE_SHORT are counted pairwise by their lane; everything longer (and every long histogram
// run) goes through a per-wave LDS table of 256 counters.
__global__ __launch_bounds__(THREADS) void hist_kernel(
    const int64_t* __restrict__ labels, const int64_t* __restrict__ pointers,
    const int64_t* __restrict__ order, int64_t num_voxels, int n_bins,
    int64_t* __restrict__ hist, int64_t* __restrict__ vote, int32_t* __restrict__ status) {
  __shared__ uint32_t table[THREADS / 64][MAX_LABEL_BINS];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < num_voxels;
       base += stride) {                                      // wave-uniform trip count
    const int64_t v = base + lane;
    int64_t b = 0, e = 0;
    if (v < num_voxels) {
      b = pointers[v];
      e = pointers[v + 1];
    }
    const int64_t len = e - b;
    const bool wide = hist ? len > LONG_RUN : len > VOTE_SHORT;
    if (v < num_voxels && !wide) {
      if (hist) {
        int64_t* row = hist + v * n_bins;
        for (int k = 0; k < n_bins; ++k) row[k] = 0;
        for (int64_t j = b; j < e; ++j) {
          const int64_t l = labels[order[j]];
          if (l < 0 || l >= n_bins) bad = true;
          else row[l] += 1;
        }
      }
      if (vote) {
        int best_count = 0;
        int64_t best = 0;
        for (int64_t j = b; j < e; ++j) {
          const int64_t l = labels[order[j]];
          if (l < 0 || l >= n_bins) {
            bad = true;
            continue;
          }
          int cnt = 0;
          for (int64_t k = b; k < e; ++k) cnt += labels[order[k]] == l;
          if (cnt > best_count || (cnt == best_count && l < best)) {
            best_count = cnt;
            best = l;
          }
        }
        vote[v] = best;
      }
    }
    uint64_t todo = __ballot(wide);
    while (todo) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const int64_t b2 = __shfl(b, src, 64), e2 = __shfl(e, src, 64);
      const int64_t v2 = base + src;
      for (int k = lane; k < MAX_LABEL_BINS; k += 64) table[w][k] = 0;
      __builtin_amdgcn_wave_barrier();
      for (int64_t j = b2 + lane; j < e2; j += 64) {
        const int64_t l = labels[order[j]];
        if (l < 0 || l >= n_bins) bad = true;
        else atomicAdd(&table[w][(int)l], 1u);               // LDS, integer: order-free
      }
      __builtin_amdgcn_wave_barrier();
      if (hist)
        for (int k = lane; k < n_bins; k += 64) hist[v2 * n_bins + k] = (int64_t)table[w][k];
      if (vote) {
        uint32_t best_count = 0;
        int best = 0;
        for (int k = lane; k < n_bins; k += 64) {            // ascending: the lowest label wins
          const uint32_t cnt = table[w][k];
          if (cnt > best_count) {
            best_count = cnt;
            best = k;
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const uint32_t oc = __shfl_xor(best_count, o, 64);
          const int ob = __shfl_xor(best, o, 64);
          if (oc > best_count || (oc == best_count && ob < best)) {
            best_count = oc;
            best = ob;
          }
        }
        if (lane == 0) vote[v2] = best;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (bad) atomicOr(status, 1);
}

__global__ __launch_bounds__(THREADS) void last_kernel(
    const int64_t* __restrict__ pointers, const int64_t* __restrict__ order, int64_t num_voxels,
    uint64_t seed, int use_seed, int64_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < num_voxels;
       base += stride) {
    const int64_t v = base + lane;
    int64_t b = 0, e = 0;
    if (v < num_voxels) {
      b = pointers[v];
      e = pointers[v + 1];
    }
    if (v < num_voxels && !use_seed) out[v] = order[e - 1];   // ascending inside the run
    if (!use_seed) continue;                                  // (wave-uniform)
    const bool longrun = e - b > LONG_RUN;
    if (v < num_voxels && !longrun) {
      uint64_t best = 0;
      for (int64_t j = b; j < e; ++j) {
        const uint64_t p = (uint64_t)order[j];
        const uint64_t cand = ((uint64_t)rand32(seed, p) << 32) | p;   // p < 2^31
        best = cand > best ? cand : best;
      }
      out[v] = (int64_t)(best & 0xffffffffull);
    }
    uint64_t todo = __ballot(longrun);
    while (todo) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const int64_t b2 = __shfl(b, src, 64), e2 = __shfl(e, src, 64);
      uint64_t best = 0;
      for (int64_t j = b2 + lane; j < e2; j += 64) {
        const uint64_t p = (uint64_t)order[j];
        const uint64_t cand = ((uint64_t)rand32(seed, p) << 32) | p;
        best = cand > best ? cand : best;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const uint64_t other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
      }
      if (lane == 0) out[base + src] = (int64_t)(best & 0xffffffffull);
    }
  }
}

}  // namespace
}  // namespace spt

using namespace spt;

extern "C" int spt_voxel_bounds_f32(const float* pos, int64_t n, int64_t ld, float size,
                                    const int64_t* batch, int32_t* record, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "n out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(pos && record, "null pointer");
  SPT_CHECK_ARG(ld >= 3, "ld must be at least 3");
  SPT_CHECK_ARG(size > 0.f && size <= 3.4028234663852886e38f, "size must be positive and finite");
  bounds_init_kernel<<<1, 64, 0, stream>>>(record, batch != nullptr);
  bounds_kernel<<<stream_grid(n, THREADS * 4), THREADS, 0, stream>>>(pos, n, ld, size, batch,
                                                                      record);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_voxel_groups_workspace_bytes(int64_t n, int key_bits) {
  if (!count_ok(n) || n < 1 || key_bits < 1 || key_bits > 63) return 0;
  return runs_plan(n, key_bits, false).total;
}

extern "C" int spt_voxel_groups_f32(const float* pos, int64_t n, int64_t ld, float size,
                                    const int64_t* batch, const int64_t* origin, const int* bits,
                                    int64_t* pointers, int64_t* cluster, int64_t* order,
                                    int64_t* last, int32_t* coords, int64_t* count, void* ws,
                                    size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "n out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(pos && origin && bits && pointers && cluster && order && last && coords && count,
                "null pointer");
  SPT_CHECK_ARG(ld >= 3, "ld must be at least 3");
  SPT_CHECK_ARG(size > 0.f && size <= 3.4028234663852886e38f, "size must be positive and finite");
  KeyLayout L;
  int key_bits = 0;
  for (int a = 0; a < 4; ++a) {
    SPT_CHECK_ARG(bits[a] >= 0 && bits[a] <= 32, "a field is wider than 32 bits");
    L.origin[a] = origin[a];
    L.bits[a] = bits[a];
    key_bits += bits[a];
  }
  SPT_CHECK_ARG(batch || bits[3] == 0, "batch bits without a batch");
  SPT_CHECK_ARG(key_bits >= 1 && key_bits <= 63, "the key needs 1 .. 63 bits");
  const RunsPlan p = runs_plan(n, key_bits, false);
  SPT_CHECK_ARG(ws && ws_bytes >= p.total, "workspace too small");
  char* base = (char*)ws;
  Runs r = runs_carve(base, p, n);

  const int g = stream_grid(n, THREADS);
  keys_kernel<<<g, THREADS, 0, stream>>>(pos, n, ld, size, batch, L, r.in.minor, r.in.major);
  SPT_CHECK_ARG(sort_runs(base, p, r, n, stream) == 0, "sort scratch too small");
  SPT_CHECK_ARG(flag_runs(base, p, r, n, NO_MAJOR_LIMIT, stream) == 0, "scan partials too small");
  groups_kernel<<<g, THREADS, 0, stream>>>(r.sorted, r.excl, n, L, pointers, cluster, order, last,
                                           coords, count);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_voxel_mean_f32(const float* x, int64_t n, int cols, int64_t ld_x,
                                  const int64_t* pointers, const int64_t* order,
                                  int64_t num_voxels, int normalize, float* out, int64_t ld_out,
                                  spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "n out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(num_voxels >= 1 && num_voxels <= n, "num_voxels out of range (1 .. n)");
  SPT_CHECK_ARG(cols >= 1 && cols <= 4096, "cols out of range (1 .. 4096)");
  SPT_CHECK_ARG(ld_x >= cols && ld_out >= cols, "a row stride is below the column count");
  SPT_CHECK_ARG(!normalize || cols == 3, "normalize needs 3 columns");
  SPT_CHECK_ARG(x && pointers && order && out, "null pointer");
  mean_kernel<<<stream_grid(num_voxels * cols, THREADS), THREADS, 0, stream>>>(
      x, cols, ld_x, pointers, order, num_voxels, out, ld_out);
  if (normalize)
    normalize3_kernel<<<stream_grid(num_voxels, THREADS), THREADS, 0, stream>>>(out, ld_out,
                                                                                 num_voxels);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_voxel_hist_i64(const int64_t* labels, int64_t n, const int64_t* pointers,
                                  const int64_t* order, int64_t num_voxels, int n_bins,
                                  int64_t* hist, int64_t* vote, int32_t* status,
                                  spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "n out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(num_voxels >= 1 && num_voxels <= n, "num_voxels out of range (1 .. n)");
  SPT_CHECK_ARG(n_bins >= 1 && n_bins <= MAX_LABEL_BINS, "n_bins out of range (1 .. 256)");
  SPT_CHECK_ARG(labels && pointers && order && status, "null pointer");
  SPT_CHECK_ARG((hist != nullptr) != (vote != nullptr), "exactly one of hist and vote");
  SPT_CHECK_ARG(hipMemsetAsync(status, 0, sizeof(int32_t), stream) == hipSuccess,
                "could not queue the status reset");
  hist_kernel<<<stream_grid(num_voxels, THREADS), THREADS, 0, stream>>>(
      labels, pointers, order, num_voxels, n_bins, hist, vote, status);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_voxel_last(const int64_t* pointers, const int64_t* order, int64_t n,
                              int64_t num_voxels, uint64_t seed, int use_seed, int64_t* out,
                              spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "n out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(num_voxels >= 1 && num_voxels <= n, "num_voxels out of range (1 .. n)");
  SPT_CHECK_ARG(pointers && order && out, "null pointer");
  last_kernel<<<stream_grid(num_voxels, THREADS), THREADS, 0, stream>>>(pointers, order,
                                                                         num_voxels, seed,
                                                                         use_seed, out);
  SPT_CHECK_LAUNCH();
  return 0;
}
