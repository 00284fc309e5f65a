// Panoptic evaluation on the device (include/spt_hip.h, "Panoptic evaluation"): merging the
// cluster-object overlaps of a level into predicted instances, the per-pair sizes / IoUs / void
// masks, the five per-class counters of PanopticQuality3D, and the weighted group mean behind
// the instances' semantic logits; and, for the panoptic criterion, the major object of every
// cluster (InstanceData.major) with its data-dependent branch kept on the device.
//
// Grouping is always ONE stable radix sort of a key as wide as its extents need and the runs of
// equal keys (csrc/sorted_runs.hpp), and integer run sums: no
// float and no atomic whose order matters takes part in an integer result.  `/` is the correctly
// rounded IEEE division (no fast-math flag on this file, no reciprocal) and (float)int64 rounds
// to nearest even, as torch converts.
//
// No value read from device memory is used as an address before it is compared with its bound:
// `pointers` of the caller are searched and compared with positions, or range-checked before a
// loop runs over them; parents, labels and predictions are range-checked before they index a
// table; sorted positions and run starts are this file's own scratch and are checked all the same.
#include "common.hpp"
#include "sorted_runs.hpp"

#include <algorithm>
#include <limits.h>

namespace spt {
namespace {

constexpr int THREADS = 256;
constexpr int LONG_RUN = 512;      // runs longer than this are reduced by a whole wave
constexpr int MAXC = 32;           // classes of the per-workgroup tables (as csrc/predict.hip)

// record of spt_merge_instances_i64 (int64 words)
enum { MR_PAIRS = 0, MR_PARENTS = 1, MR_BAD_PARENT = 2, MR_BAD_PAIR = 3 };
// status of spt_pair_stats_i64 / spt_panoptic_counts_i64 (int32 words)
enum { ST_POINTERS = 0, ST_OBJ = 1, ST_PRED = 2, ST_IOU = 3 };

inline bool count_ok(int64_t n) { return n >= 0 && n < (int64_t)INT32_MAX; }

// largest v in [lo, hi] with p[v] <= j; lo when there is none
__device__ __forceinline__ int64_t last_not_above(const int64_t* __restrict__ p, int64_t lo,
                                                  int64_t hi, int64_t j) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (p[mid] <= j) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// cluster of pair position j (pointers are only compared); *ok: the cluster claims j
__device__ __forceinline__ int64_t cluster_of(const int64_t* __restrict__ pointers, int64_t G,
                                              int64_t j, bool* ok) {
  const int64_t v = last_not_above(pointers, 0, G - 1, j);
  *ok = pointers[v] <= j && j < pointers[v + 1];
  return v;
}

__device__ __forceinline__ void add64(int64_t* p, int64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// Lane `r` owns run [b, e): a short run is reduced and finished by its lane, a long one by the
// whole wave, one after the other.  load(j, s, m) adds position j into the K sums `s` and the
// maximum `m`; done(r, b, e, s, m, first, step) finishes: it loops j = b + first; j < e; j += step
// for per-position writes and does its single writes under first == 0.  Every lane of a wave
// must call this (wave-uniform trip counts at the call site).
template <int K, typename Load, typename Done>
__device__ __forceinline__ void reduce_runs(int64_t r, bool valid, int64_t b, int64_t e,
                                            Load load, Done done) {
  const int lane = threadIdx.x & 63;
  const bool longrun = valid && e - b > LONG_RUN;
  if (valid && !longrun) {
    int64_t s[K], m = -1;
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0;
    for (int64_t j = b; j < e; ++j) load(j, s, m);
    done(r, b, e, s, m, 0, 1);
  }
  uint64_t todo = __ballot(longrun);
  while (todo) {
    const int src = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1;
    const int64_t b2 = __shfl(b, src, 64), e2 = __shfl(e, src, 64), r2 = __shfl(r, src, 64);
    int64_t s[K], m = -1;
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0;
    for (int64_t j = b2 + lane; j < e2; j += 64) load(j, s, m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < K; ++k) s[k] += __shfl_xor(s[k], o, 64);     // integers: order-free
      const int64_t om = __shfl_xor(m, o, 64);
      m = om > m ? om : m;
    }
    done(r2, b2, e2, s, m, lane, 64);
  }
}

// ---- extents -----------------------------------------------------------------------------------
__global__ void extents_init_kernel(int64_t* __restrict__ rec) {
  if (threadIdx.x < 4) rec[threadIdx.x] = (threadIdx.x & 1) ? INT64_MIN : INT64_MAX;
}

__global__ __launch_bounds__(THREADS) void extents_kernel(
    const int64_t* __restrict__ obj, int64_t P, const int64_t* __restrict__ idx, int64_t G,
    int64_t* __restrict__ rec) {
  int64_t lo[2] = {INT64_MAX, INT64_MAX}, hi[2] = {INT64_MIN, INT64_MIN};
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < P; i += stride) {
    const int64_t v = obj[i];
    lo[0] = v < lo[0] ? v : lo[0];
    hi[0] = v > hi[0] ? v : hi[0];
  }
  if (idx)
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < G; i += stride) {
      const int64_t v = idx[i];
      lo[1] = v < lo[1] ? v : lo[1];
      hi[1] = v > hi[1] ? v : hi[1];
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int64_t l = __shfl_xor(lo[a], o, 64), h = __shfl_xor(hi[a], o, 64);
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = h > hi[a] ? h : hi[a];
    }
  if ((threadIdx.x & 63) == 0)                 // minimum / maximum: the order does not matter
    for (int a = 0; a < (idx ? 2 : 1); ++a) {
      atomicMin(reinterpret_cast<long long*>(rec) + 2 * a, (long long)lo[a]);
      atomicMax(reinterpret_cast<long long*>(rec) + 2 * a + 1, (long long)hi[a]);
    }
}

// ---- keys --------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t obj_field(int64_t o, int64_t obj_lo, int obj_bits, bool* bad) {
  const uint64_t rel = (uint64_t)o - (uint64_t)obj_lo;
  const uint64_t mask = (~0ull) >> (64 - obj_bits);               // 1 <= obj_bits <= 63
  *bad = o < obj_lo || (rel & ~mask) != 0;
  return rel & mask;
}

// merge: key = (parent, obj - obj_lo), the object in the low bits
__global__ __launch_bounds__(THREADS) void merge_keys_kernel(
    const int64_t* __restrict__ pointers, const int64_t* __restrict__ obj,
    const int64_t* __restrict__ idx, int64_t G, int64_t P, int64_t num_parents, int64_t obj_lo,
    int obj_bits, uint32_t* __restrict__ lo32, uint32_t* __restrict__ hi32,
    int32_t* __restrict__ pair_parent, int64_t* __restrict__ rec) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t j = (int64_t)blockIdx.x * THREADS + threadIdx.x; j < P; j += stride) {
    bool ok, bad;
    const int64_t v = cluster_of(pointers, G, j, &ok);
    int64_t par = idx[v];
    if (par < 0 || par >= num_parents) {
      add64(&rec[MR_BAD_PARENT], 1);
      par = 0;
    }
    const uint64_t field = obj_field(obj[j], obj_lo, obj_bits, &bad);
    if (!ok || bad) add64(&rec[MR_BAD_PAIR], 1);
    const uint64_t key = ((uint64_t)par << obj_bits) | field;
    lo32[j] = (uint32_t)key;
    if (hi32) hi32[j] = (uint32_t)(key >> 32);
    pair_parent[j] = (int32_t)par;
  }
}

// ---- merge: one lane per run of equal (parent, obj) ---------------------------------------------
__global__ __launch_bounds__(THREADS) void merge_runs_kernel(
    const int64_t* __restrict__ obj, const int64_t* __restrict__ count,
    const int64_t* __restrict__ y, const uint32_t* __restrict__ order32,
    const int32_t* __restrict__ run_start, const uint32_t* __restrict__ num_runs,
    const int32_t* __restrict__ pair_parent, int64_t n, int64_t num_parents,
    int64_t* __restrict__ out_pointers, int64_t* __restrict__ out_obj,
    int64_t* __restrict__ out_count, int64_t* __restrict__ out_y, int64_t* __restrict__ rec) {
  const int lane = threadIdx.x & 63;
  int64_t R = *num_runs;
  R = R < n ? R : n;
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t base = (int64_t)blockIdx.x * THREADS + (threadIdx.x & ~63); base < R;
       base += stride) {                                      // wave-uniform trip count
    const int64_t r = base + lane;
    int64_t b = 0, e = 0;
    bool valid = r < R;
    if (valid) {
      b = run_start[r];
      e = run_start[r + 1];
      valid = 0 <= b && b < e && e <= n;
    }
    reduce_runs<1>(
        r, valid, b, e,
        [&](int64_t j, int64_t* s, int64_t&) {
          const int64_t p = order32[j];
          if (p < n) s[0] += count[p];
        },
        [&](int64_t r_, int64_t b_, int64_t e_, const int64_t* s, int64_t, int first, int) {
          if (first != 0) return;
          const int64_t p0 = order32[b_], pl = order32[e_ - 1];
          if (p0 >= n || pl >= n) return;
          out_obj[r_] = obj[p0];
          out_count[r_] = s[0];
          out_y[r_] = y[pl];                                   // the last pair holding the key
          int64_t par = pair_parent[p0], prev = -1;            // both in [0, num_parents)
          if (b_ > 0) {
            const int64_t pp = order32[b_ - 1];
            prev = pp < n ? pair_parent[pp] : -1;
          }
          if (par < 0 || par >= num_parents || prev >= par + 1) return;
          for (int64_t q = prev + 1; q <= par; ++q) out_pointers[q] = r_;
          if (par != prev) add64(&rec[MR_PARENTS], 1);
          if (e_ == n) {
            for (int64_t q = par + 1; q <= num_parents; ++q) out_pointers[q] = r_ + 1;
            add64(&rec[MR_PAIRS], r_ + 1);
          }
        });
  }
}

// ---- pair statistics ---------------------------------------------------------------------------
// one lane per cluster: size, void size, void mask
__global__ __launch_bounds__(THREADS) void cluster_sizes_kernel(
    const int64_t* __restrict__ pointers, const int64_t* __restrict__ count,
    const int64_t* __restrict__ y, int64_t G, int64_t P, int C, int64_t* __restrict__ cl_size,
    int64_t* __restrict__ cl_void, uint8_t* __restrict__ cluster_void,
    int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && threadIdx.x == 0 && (pointers[0] != 0 || pointers[G] != P))
    atomicAdd(&status[ST_POINTERS], 1);
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t base = (int64_t)blockIdx.x * THREADS + (threadIdx.x & ~63); base < G;
       base += stride) {
    const int64_t v = base + lane;
    int64_t b = 0, e = 0;
    bool valid = v < G;
    if (valid) {
      b = pointers[v];
      e = pointers[v + 1];
      if (!(0 <= b && b <= e && e <= P)) {
        atomicAdd(&status[ST_POINTERS], 1);
        b = e = 0;                                             // an empty cluster
      }
    }
    reduce_runs<2>(
        v, valid, b, e,
        [&](int64_t j, int64_t* s, int64_t&) {
          const int64_t c = count[j], l = y[j];
          s[0] += c;
          s[1] += (l < 0 || l >= C) ? c : 0;
        },
        [&](int64_t v_, int64_t, int64_t, const int64_t* s, int64_t, int first, int) {
          if (first != 0) return;
          cl_size[v_] = s[0];
          cl_void[v_] = s[1];
          cluster_void[v_] = (float)s[1] / (float)s[0] > 0.5f ? 1 : 0;   // 0 / 0 = NaN: not void
        });
  }
}

__global__ __launch_bounds__(THREADS) void stats_keys_kernel(
    const int64_t* __restrict__ pointers, const int64_t* __restrict__ obj,
    const int64_t* __restrict__ y, int64_t G, int64_t P, int C, int64_t obj_lo, int obj_bits,
    const int64_t* __restrict__ cl_size, const uint8_t* __restrict__ cluster_void,
    uint32_t* __restrict__ lo32, uint32_t* __restrict__ hi32, int32_t* __restrict__ pair_cluster,
    int64_t* __restrict__ a_size, uint8_t* __restrict__ pair_void, int32_t* __restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t j = (int64_t)blockIdx.x * THREADS + threadIdx.x; j < P; j += stride) {
    bool ok, bad;
    const int64_t v = cluster_of(pointers, G, j, &ok);
    if (!ok) atomicAdd(&status[ST_POINTERS], 1);
    const uint64_t key = obj_field(obj[j], obj_lo, obj_bits, &bad);
    if (bad) atomicAdd(&status[ST_OBJ], 1);
    lo32[j] = (uint32_t)key;
    if (hi32) hi32[j] = (uint32_t)(key >> 32);
    pair_cluster[j] = (int32_t)v;
    a_size[j] = cl_size[v];
    const int64_t l = y[j];
    pair_void[j] = (l < 0 || l >= C || cluster_void[v]) ? 1 : 0;
  }
}

// one lane per run of equal obj
__global__ __launch_bounds__(THREADS) void object_runs_kernel(
    const int64_t* __restrict__ count, const int64_t* __restrict__ cropped_in,
    const uint32_t* __restrict__ order32, const int32_t* __restrict__ run_start,
    const uint32_t* __restrict__ num_runs, const int32_t* __restrict__ pair_cluster,
    const int64_t* __restrict__ cl_size, const int64_t* __restrict__ cl_void,
    const uint8_t* __restrict__ cluster_void, const uint8_t* __restrict__ pair_void,
    const int64_t* __restrict__ a_size, int64_t n, int64_t G, int64_t* __restrict__ b_size,
    float* __restrict__ iou, int64_t* __restrict__ pair_cropped, float* __restrict__ kept_iou,
    uint8_t* __restrict__ gt_head) {
  const int lane = threadIdx.x & 63;
  int64_t R = *num_runs;
  R = R < n ? R : n;
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t base = (int64_t)blockIdx.x * THREADS + (threadIdx.x & ~63); base < R;
       base += stride) {
    const int64_t r = base + lane;
    int64_t b = 0, e = 0;
    bool valid = r < R;
    if (valid) {
      b = run_start[r];
      e = run_start[r + 1];
      valid = 0 <= b && b < e && e <= n;
    }
    reduce_runs<2>(
        r, valid, b, e,
        [&](int64_t j, int64_t* s, int64_t& m) {
          const int64_t p = order32[j];
          if (p >= n) return;
          const int64_t c = count[p], v = pair_cluster[p];
          s[0] += c;
          s[1] += (v >= 0 && v < G && cluster_void[v]) ? c : 0;
          if (!pair_void[p]) m = p > m ? p : m;                 // the last pair kept
        },
        [&](int64_t, int64_t b_, int64_t e_, const int64_t* s, int64_t m, int first, int step) {
          for (int64_t j = b_ + first; j < e_; j += step) {
            const int64_t p = order32[j];
            if (p >= n) continue;
            const int64_t c = count[p], v = pair_cluster[p];
            const int64_t bs = s[0] + (cropped_in ? cropped_in[p] : 0);
            b_size[p] = bs;
            pair_cropped[p] = s[1];
            iou[p] = (float)c / (float)(a_size[p] + bs - c);
            float k = 0.f;     // after void removal: the cluster without its void pairs, the
                               // object whole (what left with void clusters comes back cropped)
            if (!pair_void[p] && v >= 0 && v < G)
              k = (float)c / (float)((cl_size[v] - cl_void[v]) + s[0] - c);
            kept_iou[p] = k;
            gt_head[p] = p == m ? 1 : 0;
          }
        });
  }
}

// ---- the five counters -------------------------------------------------------------------------
// tables of one workgroup: tp, gt, pred, then (hi, lo) of the two fixed-point IoU sums
enum { T_TP = 0, T_GT, T_PRED, T_SUM_HI, T_SUM_LO, T_MOD_HI, T_MOD_LO, T_ROWS };

// iou in [0, 1] as hi * 2^-32 + lo * 2^-64, exact for every f32 down to 2^-40 (floor below)
__device__ __forceinline__ void fixed_point(float iou, unsigned long long* hi,
                                            unsigned long long* lo) {
  const double d = (double)iou * 4294967296.0;
  *hi = (unsigned long long)d;
  *lo = (unsigned long long)((d - (double)*hi) * 4294967296.0);
}

__global__ __launch_bounds__(THREADS) void counts_kernel(
    const int64_t* __restrict__ pred_sem, const int64_t* __restrict__ pointers,
    const int64_t* __restrict__ y, const uint8_t* __restrict__ pair_void,
    const float* __restrict__ kept_iou, const uint8_t* __restrict__ gt_head,
    const uint8_t* __restrict__ cluster_void, int64_t G, int64_t P, int C,
    const uint8_t* __restrict__ stuff, int64_t* __restrict__ state,
    unsigned long long* __restrict__ sums, int32_t* __restrict__ status) {
  __shared__ unsigned long long t[T_ROWS][MAXC];
  for (int i = threadIdx.x; i < T_ROWS * MAXC; i += THREADS) (&t[0][0])[i] = 0ull;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t j = (int64_t)blockIdx.x * THREADS + threadIdx.x; j < P; j += stride) {
    if (pair_void[j]) continue;
    const int64_t l = y[j];
    if (l < 0 || l >= C) continue;                              // (void: cannot be kept)
    bool ok;
    const int64_t v = cluster_of(pointers, G, j, &ok);
    if (!ok) {
      atomicAdd(&status[ST_POINTERS], 1);
      continue;
    }
    if (gt_head[j]) atomicAdd(&t[T_GT][l], 1ull);
    if (pred_sem[v] != l) continue;
    const float q = kept_iou[j];
    if (!(q >= 0.f && q <= 1.f)) {                              // NaN (an empty union)
      atomicAdd(&status[ST_IOU], 1);
      continue;
    }
    const bool tp = q > 0.5f;
    if (!tp && !stuff[l]) continue;
    unsigned long long hi, lo;
    fixed_point(q, &hi, &lo);
    if (tp) {
      atomicAdd(&t[T_TP][l], 1ull);
      atomicAdd(&t[T_SUM_HI][l], hi);
      atomicAdd(&t[T_SUM_LO][l], lo);
    }
    atomicAdd(&t[T_MOD_HI][l], hi);
    atomicAdd(&t[T_MOD_LO][l], lo);
  }
  for (int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x; v < G; v += stride) {
    if (cluster_void[v]) continue;
    const int64_t ps = pred_sem[v];
    if (ps < 0 || ps >= C) atomicAdd(&status[ST_PRED], 1);
    else atomicAdd(&t[T_PRED][ps], 1ull);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T_ROWS * C; i += THREADS) {
    const int row = i / C, c = i - row * C;
    const unsigned long long v = t[row][c];
    if (!v) continue;
    if (row <= T_PRED) atomicAdd(reinterpret_cast<unsigned long long*>(state) + row * C + c, v);
    else atomicAdd(&sums[(row - T_SUM_HI) * C + c], v);
  }
}

// state f64 rows 3 and 4 += the call's fixed-point sums: one add per class and call
__global__ void counts_finish_kernel(const unsigned long long* __restrict__ sums, int C,
                                     int64_t* __restrict__ state) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double* f = reinterpret_cast<double*>(state);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double add = (double)sums[(2 * k) * C + c] * 2.3283064365386963e-10 +      // 2^-32
                       (double)sums[(2 * k + 1) * C + c] * 5.421010862427522e-20;    // 2^-64
    f[(3 + k) * C + c] = f[(3 + k) * C + c] + add;
  }
}

// ---- weighted group mean -----------------------------------------------------------------------
__global__ void group_keys_kernel(const int64_t* __restrict__ idx, int64_t n, int64_t num_groups,
                                  uint32_t* __restrict__ keys, int32_t* __restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int64_t g = idx[i];
    if (g < 0 || g >= num_groups) {
      atomicAdd(&status[0], 1);
      g = num_groups;                                           // a group of its own, not written
    }
    keys[i] = (uint32_t)g;
  }
}

// One lane per (group, column).  Up to LONG_RUN rows: s = 0; s = s + round(x * w) in ascending
// row order (the stable sort keeps it) - scatter_sum on the CPU bit for bit.  Longer: exact f64
// products, 64 strided f64 partial sums, a fixed butterfly and ONE rounding to f32 at the end:
// deterministic, and within an f32 ulp of the true mean where an f32 tree is not.
__global__ __launch_bounds__(THREADS) void weighted_mean_kernel(
    const float* __restrict__ x, const float* __restrict__ w, int64_t n, int cols,
    const int32_t* __restrict__ rowptr, const uint32_t* __restrict__ order32, int64_t num_groups,
    float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t total = num_groups * cols;
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t base = (int64_t)blockIdx.x * THREADS + (threadIdx.x & ~63); base < total;
       base += stride) {
    const int64_t t = base + lane;
    int64_t g = 0, b = 0, e = 0;
    int c = 0;
    bool valid = t < total;
    if (valid) {
      g = t / cols;
      c = (int)(t - g * cols);
      b = rowptr[g];
      e = rowptr[g + 1];
      if (!(0 <= b && b <= e && e <= n)) b = e = 0;
    }
    const bool longrun = valid && e - b > LONG_RUN;
    if (valid && !longrun) {
      float s = 0.0f, ws = 0.0f;
      for (int64_t j = b; j < e; ++j) {
        const int64_t p = order32[j];
        if (p >= n) continue;
        const float wp = w[p];
        const float prod = x[p * cols + c] * wp;                // rounded before it is added
        s = s + prod;
        ws = ws + wp;
      }
      if (ws == 0.0f) ws = 1.0f;
      out[g * cols + c] = s / ws;
    }
    uint64_t todo = __ballot(longrun);
    while (todo) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const int64_t b2 = __shfl(b, src, 64), e2 = __shfl(e, src, 64), g2 = __shfl(g, src, 64);
      const int c2 = __shfl(c, src, 64);
      double s = 0.0, ws = 0.0;
      for (int64_t j = b2 + lane; j < e2; j += 64) {
        const int64_t p = order32[j];
        if (p >= n) continue;
        const double wp = (double)w[p];
        s = s + (double)x[p * cols + c2] * wp;                  // exact: 24 x 24 bits
        ws = ws + wp;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {                        // fixed tree
        s = s + __shfl_xor(s, o, 64);
        ws = ws + __shfl_xor(ws, o, 64);
      }
      if (ws == 0.0) ws = 1.0;
      if (lane == 0) out[g2 * cols + c2] = (float)(s / ws);     // the one rounding to f32
    }
  }
}

// ---- major objects (InstanceData.major, src/data/instance.py:162-225) ------------------------------
// status of spt_instance_major_i64 (int32 words)
enum { MJ_EMPTY = 0, MJ_POINTERS = 1 };
constexpr int MAJOR_WAVE = 64;     // clusters of more pairs than this are searched by a whole wave

// the largest value, and among equal values the lowest pair index (scatter_max on the CPU)
struct Best {
  int64_t c, j;
};
__device__ __forceinline__ void take_best(Best& b, int64_t c, int64_t j) {
  if (c > b.c || (c == b.c && j < b.j)) {
    b.c = c;
    b.j = j;
  }
}

// Kernel 1: both candidates of every cluster - the pair of the largest count (into the outputs)
// and the pair of the largest count * ~void (into scratch) - and the flag "some cluster whose
// largest pair is void holds it with count / total <= 0.5 (as f32)".
__global__ __launch_bounds__(THREADS) void major_candidates_kernel(
    const int64_t* __restrict__ pointers, const int64_t* __restrict__ obj,
    const int64_t* __restrict__ count, const int64_t* __restrict__ y, int64_t G, int64_t P, int C,
    int64_t* __restrict__ out_obj, int64_t* __restrict__ out_count, int64_t* __restrict__ out_y,
    int64_t* __restrict__ nv_obj, int64_t* __restrict__ nv_count, int64_t* __restrict__ nv_y,
    int32_t* __restrict__ flag, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && threadIdx.x == 0 && (pointers[0] != 0 || pointers[G] != P))
    atomicAdd(&status[MJ_POINTERS], 1);
  auto load = [&](int64_t j, Best& m, Best& n, int64_t& total) {
    const int64_t c = count[j], l = y[j];
    total += c;
    take_best(m, c, j);
    take_best(n, (l < 0 || l >= C) ? 0 : c, j);
  };
  // writes both candidates of cluster v; true when v raises the flag
  auto finish = [&](int64_t v, const Best& m, const Best& n, int64_t total) -> bool {
    if (m.j < 0 || m.j >= P || n.j < 0 || n.j >= P) {      // no pair: nothing to index
      out_obj[v] = nv_obj[v] = -1;
      out_count[v] = nv_count[v] = 0;
      out_y[v] = nv_y[v] = -1;
      return false;
    }
    const int64_t ym = y[m.j];
    out_obj[v] = obj[m.j];
    out_count[v] = m.c;
    out_y[v] = ym;
    nv_obj[v] = obj[n.j];
    nv_count[v] = n.c;
    nv_y[v] = y[n.j];
    // (0 / 0 = NaN is not above one half either)
    return (ym < 0 || ym >= C) && !((float)m.c / (float)total > 0.5f);
  };
  bool up = false;
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t base = (int64_t)blockIdx.x * THREADS + (threadIdx.x & ~63); base < G;
       base += stride) {                                      // wave-uniform trip count
    const int64_t v = base + lane;
    int64_t b = 0, e = 0;
    const bool valid = v < G;
    if (valid) {
      b = pointers[v];
      e = pointers[v + 1];
      if (!(0 <= b && b <= e && e <= P)) {
        atomicAdd(&status[MJ_POINTERS], 1);
        b = e = 0;
      } else if (b == e) {
        atomicAdd(&status[MJ_EMPTY], 1);                       // the reference indexes out of range
      }
    }
    const bool longrun = valid && e - b > MAJOR_WAVE;
    if (valid && !longrun) {
      Best m = {INT64_MIN, INT64_MAX}, n = {INT64_MIN, INT64_MAX};
      int64_t total = 0;
      for (int64_t j = b; j < e; ++j) load(j, m, n, total);
      up = finish(v, m, n, total) || up;
    }
    uint64_t todo = __ballot(longrun);
    while (todo) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const int64_t b2 = __shfl(b, src, 64), e2 = __shfl(e, src, 64), v2 = __shfl(v, src, 64);
      Best m = {INT64_MIN, INT64_MAX}, n = {INT64_MIN, INT64_MAX};
      int64_t total = 0;
      for (int64_t j = b2 + lane; j < e2; j += 64) load(j, m, n, total);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        total += __shfl_xor(total, o, 64);                     // integers: order-free
        take_best(m, __shfl_xor(m.c, o, 64), __shfl_xor(m.j, o, 64));
        take_best(n, __shfl_xor(n.c, o, 64), __shfl_xor(n.j, o, 64));
      }
      if (lane == 0) up = finish(v2, m, n, total) || up;
    }
  }
  // (the loop's trip count is wave-uniform: the wave is whole here) one atomic per wave at most
  if (__ballot(up) && lane == 0) atomicOr(flag, 1);
}

// Kernel 2: with the flag up EVERY cluster whose largest pair is void takes its non-void
// candidate - those above one half included, as the reference's masked assignment does.
__global__ __launch_bounds__(THREADS) void major_select_kernel(
    const int32_t* __restrict__ flag, const int64_t* __restrict__ nv_obj,
    const int64_t* __restrict__ nv_count, const int64_t* __restrict__ nv_y, int64_t G, int C,
    int64_t* __restrict__ out_obj, int64_t* __restrict__ out_count, int64_t* __restrict__ out_y) {
  if (!*flag) return;
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x; v < G; v += stride) {
    const int64_t l = out_y[v];
    if (l < 0 || l >= C) {
      out_obj[v] = nv_obj[v];
      out_count[v] = nv_count[v];
      out_y[v] = nv_y[v];
    }
  }
}

struct MajorPlan {
  size_t off_flag, off_obj, off_count, off_y, total;
};
MajorPlan major_plan(int64_t G) {
  MajorPlan m;
  const size_t nb = align_up((size_t)(G > 0 ? G : 1) * 8, 256);
  size_t off = 0;
  m.off_flag = off; off += 256;
  m.off_obj = off; off += nb;
  m.off_count = off; off += nb;
  m.off_y = off; off += nb;
  m.total = off;
  return m;
}

// ---- the entries' scratch: sort + runs (csrc/sorted_runs.hpp), then their own regions -------------
struct MergePlan {
  RunsPlan runs;
  size_t off_parent, total;
};
MergePlan merge_plan(int64_t P, int key_bits) {
  MergePlan m;
  m.runs = runs_plan(P, key_bits, true);
  m.off_parent = m.runs.total;
  m.total = m.off_parent + align_up((size_t)(P > 0 ? P : 1) * 4, 256);
  return m;
}

struct StatsPlan {
  RunsPlan runs;
  size_t off_cluster, off_size, off_void, total;
};
StatsPlan stats_plan(int64_t P, int64_t G, int key_bits) {
  StatsPlan m;
  m.runs = runs_plan(P, key_bits, true);
  size_t off = m.runs.total;
  m.off_cluster = off; off += align_up((size_t)(P > 0 ? P : 1) * 4, 256);
  m.off_size = off; off += align_up((size_t)(G > 0 ? G : 1) * 8, 256);
  m.off_void = off; off += align_up((size_t)(G > 0 ? G : 1) * 8, 256);
  m.total = off;
  return m;
}

struct MeanPlan {
  size_t off_keys, off_order, off_rowptr, off_sort, total;
};
MeanPlan mean_plan(int64_t n, int64_t num_groups) {
  MeanPlan m;
  const size_t nb = align_up((size_t)(n > 0 ? n : 1) * 4, 256);
  size_t off = 0;
  m.off_keys = off; off += nb;
  m.off_order = off; off += nb;
  m.off_rowptr = off; off += align_up((size_t)(num_groups + 2) * 4, 256);
  m.off_sort = off; off += RadixScratch::bytes(n);
  m.total = off;
  return m;
}

}  // namespace
}  // namespace spt

using namespace spt;

extern "C" int spt_instance_extents_i64(const int64_t* obj, int64_t P, const int64_t* idx,
                                        int64_t G, int64_t* record, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(P) && count_ok(G), "size out of range (0 <= n < 2^31 - 1)");
  SPT_CHECK_ARG(record && (obj || P == 0) && (idx || G == 0), "null pointer");
  extents_init_kernel<<<1, 64, 0, stream>>>(record);
  const int64_t n = P > G ? P : G;
  if (n > 0)
    extents_kernel<<<stream_grid(n, THREADS * 4), THREADS, 0, stream>>>(obj, P, idx, idx ? G : 0,
                                                                         record);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_merge_instances_workspace_bytes(int64_t P, int key_bits) {
  if (!count_ok(P) || P < 1 || key_bits < 1 || key_bits > 63) return 0;
  return merge_plan(P, key_bits).total;
}

extern "C" int spt_merge_instances_i64(const int64_t* pointers, const int64_t* obj,
                                       const int64_t* count, const int64_t* y, const int64_t* idx,
                                       int64_t G, int64_t P, int64_t num_parents, int64_t obj_lo,
                                       int obj_bits, int64_t* out_pointers, int64_t* out_obj,
                                       int64_t* out_count, int64_t* out_y, int64_t* record,
                                       void* ws, size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(P) && P >= 1 && count_ok(G) && G >= 1, "P and G in 1 .. 2^31 - 2");
  SPT_CHECK_ARG(num_parents >= 1 && num_parents <= G, "num_parents out of range (1 .. G)");
  SPT_CHECK_ARG(obj_bits >= 1 && obj_bits <= 62, "obj_bits out of range (1 .. 62)");
  const int key_bits = obj_bits + bits_for(num_parents);
  SPT_CHECK_ARG(key_bits <= 63, "the (parent, obj) key needs more than 63 bits");
  SPT_CHECK_ARG(pointers && obj && count && y && idx && out_pointers && out_obj && out_count &&
                    out_y && record, "null pointer");
  const MergePlan m = merge_plan(P, key_bits);
  SPT_CHECK_ARG(ws && ws_bytes >= m.total, "workspace too small");
  char* base = (char*)ws;
  Runs r = runs_carve(base, m.runs, P);
  int32_t* pair_parent = (int32_t*)(base + m.off_parent);
  const int g = stream_grid(P, THREADS);
  merge_keys_kernel<<<g, THREADS, 0, stream>>>(pointers, obj, idx, G, P, num_parents, obj_lo,
                                               obj_bits, r.in.minor, r.in.major, pair_parent,
                                               record);
  SPT_CHECK_ARG(find_runs(base, m.runs, r, P, NO_MAJOR_LIMIT, stream) == 0,
                "sort scratch too small");
  merge_runs_kernel<<<g, THREADS, 0, stream>>>(obj, count, y, r.sorted.order, r.run_start,
                                               r.num_runs, pair_parent, P, num_parents,
                                               out_pointers, out_obj, out_count, out_y, record);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_pair_stats_workspace_bytes(int64_t P, int64_t G, int key_bits) {
  if (!count_ok(P) || P < 1 || !count_ok(G) || G < 1 || key_bits < 1 || key_bits > 63) return 0;
  return stats_plan(P, G, key_bits).total;
}

extern "C" int spt_pair_stats_i64(const int64_t* pointers, const int64_t* obj,
                                  const int64_t* count, const int64_t* y,
                                  const int64_t* cropped_in, int64_t G, int64_t P, int C,
                                  int64_t obj_lo, int obj_bits, int64_t* a_size, int64_t* b_size,
                                  float* iou, uint8_t* cluster_void, uint8_t* pair_void,
                                  int64_t* pair_cropped, float* kept_iou, uint8_t* gt_head,
                                  int32_t* status, void* ws, size_t ws_bytes,
                                  spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(P) && P >= 1 && count_ok(G) && G >= 1, "P and G in 1 .. 2^31 - 2");
  SPT_CHECK_ARG(C >= 1, "C >= 1");
  SPT_CHECK_ARG(obj_bits >= 1 && obj_bits <= 63, "obj_bits out of range (1 .. 63)");
  SPT_CHECK_ARG(pointers && obj && count && y && a_size && b_size && iou && cluster_void &&
                    pair_void && pair_cropped && kept_iou && gt_head && status, "null pointer");
  const StatsPlan m = stats_plan(P, G, obj_bits);
  SPT_CHECK_ARG(ws && ws_bytes >= m.total, "workspace too small");
  char* base = (char*)ws;
  Runs r = runs_carve(base, m.runs, P);
  int32_t* pair_cluster = (int32_t*)(base + m.off_cluster);
  int64_t* cl_size = (int64_t*)(base + m.off_size);
  int64_t* cl_void = (int64_t*)(base + m.off_void);
  const int g = stream_grid(P, THREADS);
  cluster_sizes_kernel<<<stream_grid(G, THREADS), THREADS, 0, stream>>>(
      pointers, count, y, G, P, C, cl_size, cl_void, cluster_void, status);
  stats_keys_kernel<<<g, THREADS, 0, stream>>>(pointers, obj, y, G, P, C, obj_lo, obj_bits,
                                               cl_size, cluster_void, r.in.minor, r.in.major,
                                               pair_cluster, a_size, pair_void, status);
  SPT_CHECK_ARG(find_runs(base, m.runs, r, P, NO_MAJOR_LIMIT, stream) == 0,
                "sort scratch too small");
  object_runs_kernel<<<g, THREADS, 0, stream>>>(count, cropped_in, r.sorted.order, r.run_start,
                                                r.num_runs, pair_cluster, cl_size, cl_void,
                                                cluster_void, pair_void, a_size, P, G, b_size, iou,
                                                pair_cropped, kept_iou, gt_head);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_panoptic_counts_workspace_bytes(int C) {
  if (C < 1 || C > MAXC) return 0;
  return align_up((size_t)4 * C * 8, 256);
}

extern "C" int spt_panoptic_counts_i64(int64_t* state, const int64_t* pred_semantic,
                                       const int64_t* pointers, const int64_t* y,
                                       const uint8_t* pair_void, const float* kept_iou,
                                       const uint8_t* gt_head, const uint8_t* cluster_void,
                                       int64_t G, int64_t P, int C, const uint8_t* stuff_mask,
                                       int32_t* status, void* ws, size_t ws_bytes,
                                       spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(P) && P >= 1 && count_ok(G) && G >= 1, "P and G in 1 .. 2^31 - 2");
  SPT_CHECK_ARG(C >= 1 && C <= MAXC, "1 <= C <= 32");
  SPT_CHECK_ARG(state && pred_semantic && pointers && y && pair_void && kept_iou && gt_head &&
                    cluster_void && stuff_mask && status, "null pointer");
  const size_t need = spt_panoptic_counts_workspace_bytes(C);
  SPT_CHECK_ARG(ws && ws_bytes >= need, "workspace too small");
  SPT_CHECK_ARG(hipMemsetAsync(ws, 0, (size_t)4 * C * 8, stream) == hipSuccess,
                "could not queue the reset of the sums");
  const int64_t n = P > G ? P : G;
  const int grid = (int)std::min<int64_t>(ceil_div(n, (int64_t)THREADS), 1024);
  counts_kernel<<<grid, THREADS, 0, stream>>>(pred_semantic, pointers, y, pair_void, kept_iou,
                                              gt_head, cluster_void, G, P, C, stuff_mask, state,
                                              (unsigned long long*)ws, status);
  counts_finish_kernel<<<1, 64, 0, stream>>>((const unsigned long long*)ws, C, state);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_weighted_group_mean_workspace_bytes(int64_t n, int64_t num_groups) {
  if (!count_ok(n) || n < 1 || !count_ok(num_groups) || num_groups < 1) return 0;
  return mean_plan(n, num_groups).total;
}

extern "C" int spt_weighted_group_mean_f32(const float* x, int64_t n, int cols,
                                           const int64_t* idx, const float* w, int64_t num_groups,
                                           float* out, int32_t* status, void* ws, size_t ws_bytes,
                                           spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(n) && n >= 1 && count_ok(num_groups) && num_groups >= 1,
                "n and num_groups in 1 .. 2^31 - 2");
  SPT_CHECK_ARG(cols >= 1 && cols <= 4096, "cols out of range (1 .. 4096)");
  SPT_CHECK_ARG(x && idx && w && out && status, "null pointer");
  const MeanPlan m = mean_plan(n, num_groups);
  SPT_CHECK_ARG(ws && ws_bytes >= m.total, "workspace too small");
  char* base = (char*)ws;
  uint32_t* keys = (uint32_t*)(base + m.off_keys);
  uint32_t* order32 = (uint32_t*)(base + m.off_order);
  int32_t* rowptr = (int32_t*)(base + m.off_rowptr);
  RadixScratch s;
  s.carve(base + m.off_sort, n);
  const int g = stream_grid(n, THREADS);
  group_keys_kernel<<<g, THREADS, 0, stream>>>(idx, n, num_groups, keys, status);
  const uint32_t *ks = nullptr, *vs = nullptr;
  SPT_CHECK_ARG(radix_sort_pairs<2>(nullptr, keys, nullptr, n, bits_for(num_groups + 1), s, order32,
                                    &ks, &vs, stream) == 0, "sort scratch too small");
  // rowptr[g] = first sorted position of a key >= g, for g in 0 .. num_groups + 1
  rowptr_from_sorted_kernel<<<stream_grid(n + 1, THREADS), THREADS, 0, stream>>>(
      ks, n, num_groups + 1, rowptr);
  weighted_mean_kernel<<<stream_grid(num_groups * cols, THREADS), THREADS, 0, stream>>>(
      x, w, n, cols, rowptr, order32, num_groups, out);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_instance_major_workspace_bytes(int64_t G) {
  if (!count_ok(G) || G < 1) return 0;
  return major_plan(G).total;
}

extern "C" int spt_instance_major_i64(const int64_t* pointers, const int64_t* obj,
                                      const int64_t* count, const int64_t* y, int64_t G, int64_t P,
                                      int C, int64_t* out_obj, int64_t* out_count, int64_t* out_y,
                                      int32_t* status, void* ws, size_t ws_bytes,
                                      spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(P) && P >= 1 && count_ok(G) && G >= 1, "P and G in 1 .. 2^31 - 2");
  SPT_CHECK_ARG(C >= 1, "C >= 1");
  SPT_CHECK_ARG(pointers && obj && count && y && out_obj && out_count && out_y && status,
                "null pointer");
  const MajorPlan m = major_plan(G);
  SPT_CHECK_ARG(ws && ws_bytes >= m.total, "workspace too small");
  char* base = (char*)ws;
  int32_t* flag = (int32_t*)(base + m.off_flag);
  SPT_CHECK_ARG(hipMemsetAsync(flag, 0, sizeof(int32_t), stream) == hipSuccess,
                "could not queue the reset of the flag");
  int64_t* nv_obj = (int64_t*)(base + m.off_obj);
  int64_t* nv_count = (int64_t*)(base + m.off_count);
  int64_t* nv_y = (int64_t*)(base + m.off_y);
  const int g = stream_grid(G, THREADS);
  major_candidates_kernel<<<g, THREADS, 0, stream>>>(pointers, obj, count, y, G, P, C, out_obj,
                                                     out_count, out_y, nv_obj, nv_count, nv_y,
                                                     flag, status);
  major_select_kernel<<<g, THREADS, 0, stream>>>(flag, nv_obj, nv_count, nv_y, G, C, out_obj,
                                                 out_count, out_y);
  SPT_CHECK_LAUNCH();
  return 0;
}
