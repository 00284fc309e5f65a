// The way back from logits to the cloud (include/spt_hip.h, "Predictions back to the cloud"):
// row argmax + void mask, multi-run logit accumulation with a run stamp, and label distribution
// through one or two hops of the hierarchy - by index tensors or straight from a Cluster - with
// the confusion matrix fused in.
//
// Every result is an integer, a boolean or an f32 formed by ONE add per element, so every
// comparison against the reference is exact.  `/` below is the correctly rounded IEEE division
// (no fast-math flag on this file) and (float)int64 rounds to nearest even, as torch converts.
//
// No value read from device memory is used as an address before it is range-checked: ids,
// indices and `points` entries are compared with their bound first, `pointers` are only ever
// COMPARED with positions (a position comes from the launch geometry and is < num_points).
#include "common.hpp"

#include <algorithm>

namespace spt {
namespace {

constexpr int THREADS = 256;
constexpr int MAXC = 32;            // classes of the fused confusion matrix (as csrc/loss.hip)
constexpr int UNROLL = 4;            // points per lane and pass of the second index hop
constexpr int ACC_LANES = 16;       // lanes that share one row of spt_rows_accumulate_f32
constexpr int TILE = 1024;          // positions of one workgroup pass of the Cluster walk
constexpr int STAGE = TILE + 2;     // pointers of one tile held in LDS

// status words of the two label entries
enum { ST_FIRST = 0, ST_SECOND = 1, ST_POINTERS = 2 };
// status words of spt_rows_accumulate_f32
enum { ST_DUPLICATE = 0, ST_RANGE = 1 };

__device__ __forceinline__ int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

__global__ __launch_bounds__(THREADS) void row_argmax_kernel(
    const float* __restrict__ logits, int64_t rows, int C, const int64_t* __restrict__ hist,
    int ncols, int64_t* __restrict__ pred, uint8_t* __restrict__ is_void) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x; r < rows; r += stride) {
    if (pred) {
      const float* z = logits + r * C;
      float best = z[0];
      int arg = 0;
      // torch.argmax: the first maximum, a NaN above everything, the first NaN
      for (int c = 1; c < C; ++c) {
        const float v = z[c];
        if (!(best != best) && (v != v || v > best)) {
          best = v;
          arg = c;
        }
      }
      pred[r] = arg;
    }
    if (hist) {
      const int64_t* h = hist + r * ncols;
      int64_t total = 0;
      for (int c = 0; c < ncols; ++c) total += h[c];
      const float q = (float)h[ncols - 1] / (float)total;     // 0 / 0 = NaN: not void
      is_void[r] = q > 0.5f ? 1 : 0;
    }
  }
}

// ACC_LANES lanes per source row; the first of them swaps the run number into the stamp and
// tells the others whether this row is theirs to add.
__global__ __launch_bounds__(THREADS) void rows_accumulate_kernel(
    float* __restrict__ acc, int64_t N, const float* __restrict__ src,
    const int64_t* __restrict__ node_id, int64_t n, int C, int32_t* __restrict__ stamp, int run,
    int32_t* __restrict__ status) {
  const int sub = threadIdx.x % ACC_LANES;
  const int64_t per_block = THREADS / ACC_LANES;
  const int64_t groups = cdiv(n, per_block);
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t i = g * per_block + threadIdx.x / ACC_LANES;
    int go = 0;
    int64_t id = 0;
    if (i < n && sub == 0) {
      id = node_id[i];
      if (id < 0 || id >= N) {
        atomicAdd(&status[ST_RANGE], 1);
      } else if (atomicExch(&stamp[id], run) == run) {
        atomicAdd(&status[ST_DUPLICATE], 1);            // the first occurrence adds this row
      } else {
        go = 1;
      }
    }
    go = __shfl(go, 0, ACC_LANES);
    id = __shfl(id, 0, ACC_LANES);
    if (go) {
      float* a = acc + id * C;
      const float* s = src + i * C;
      for (int c = sub; c < C; c += ACC_LANES) a[c] = a[c] + s[c];
    }
  }
}

__device__ __forceinline__ void tally(unsigned long long* s_cm, int C, int64_t t, int64_t v) {
  if (t >= 0 && t < C && v >= 0 && v < C) atomicAdd(&s_cm[(int)t * C + (int)v], 1ull);
}

__device__ __forceinline__ void flush(const unsigned long long* s_cm, int C,
                                      int64_t* __restrict__ confmat) {
  __syncthreads();
  for (int i = threadIdx.x; i < C * C; i += THREADS)
    if (s_cm[i]) atomicAdd(reinterpret_cast<unsigned long long*>(confmat) + i, s_cm[i]);
}

__global__ __launch_bounds__(THREADS) void labels_by_index_kernel(
    const int64_t* __restrict__ label, int64_t num_label, const int64_t* __restrict__ idx_a,
    int64_t n_a, const int64_t* __restrict__ idx_b, int64_t n_b, int64_t* __restrict__ out_a,
    int64_t* __restrict__ out_b, const int64_t* __restrict__ target, int C,
    int64_t* __restrict__ confmat, int32_t* __restrict__ status) {
  __shared__ unsigned long long s_cm[MAXC * MAXC];
  if (confmat) {
    for (int i = threadIdx.x; i < C * C; i += THREADS) s_cm[i] = 0ull;
    __syncthreads();
  }
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  // first hop (without a second hop, or when its labels are wanted, it also writes and tallies;
  // otherwise it only counts the entries of idx_a out of range)
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n_a; i += stride) {
    const int64_t a = idx_a[i];
    const bool ok = a >= 0 && a < num_label;
    if (!ok) atomicAdd(&status[ST_FIRST], 1);
    if (out_a || !idx_b) {
      const int64_t v = ok ? label[a] : -1;
      if (out_a) out_a[i] = v;
      if (confmat && !idx_b) tally(s_cm, C, target[i], v);
    }
  }
  // second hop, UNROLL points per lane and pass: the three dependent loads of a point (idx_b,
  // idx_a, label) overlap with those of the lane's other points
  if (idx_b) {
    for (int64_t base = (int64_t)blockIdx.x * (THREADS * UNROLL) + threadIdx.x; base < n_b;
         base += stride * UNROLL) {
      int64_t b[UNROLL], a[UNROLL], v[UNROLL];
#pragma unroll
      for (int k = 0; k < UNROLL; ++k) {
        const int64_t p = base + (int64_t)k * THREADS;
        b[k] = p < n_b ? idx_b[p] : 0;
      }
#pragma unroll
      for (int k = 0; k < UNROLL; ++k) a[k] = b[k] >= 0 && b[k] < n_a ? idx_a[b[k]] : -1;
#pragma unroll
      for (int k = 0; k < UNROLL; ++k)      // (an idx_a entry out of range was counted above)
        v[k] = a[k] >= 0 && a[k] < num_label ? label[a[k]] : -1;
#pragma unroll
      for (int k = 0; k < UNROLL; ++k) {
        const int64_t p = base + (int64_t)k * THREADS;
        if (p < n_b) {
          if (b[k] < 0 || b[k] >= n_a) atomicAdd(&status[ST_SECOND], 1);
          if (out_b) out_b[p] = v[k];
          if (confmat) tally(s_cm, C, target[p], v[k]);
        }
      }
    }
  }
  if (confmat) flush(s_cm, C, confmat);
}

// largest v in [lo, hi] with p[v] <= j; lo when there is none
template <typename P>
__device__ __forceinline__ int64_t last_not_above(P p, int64_t lo, int64_t hi, int64_t j) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (p[mid] <= j) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The work is cut by POSITIONS of `points`, TILE at a time: one search of `pointers` for the
// tile's first cluster and one for its last, the pointers in between staged in LDS, then every
// lane finds the cluster of its position there.  Reads of `points` are coalesced and a cluster
// of thousands of points costs what thousands of singletons cost.
__global__ __launch_bounds__(THREADS) void labels_by_cluster_kernel(
    const int64_t* __restrict__ label, int64_t num_label, const int64_t* __restrict__ idx_a,
    const int64_t* __restrict__ pointers, const int64_t* __restrict__ points,
    int64_t num_clusters, int64_t num_points, int64_t* __restrict__ out,
    const int64_t* __restrict__ target, int C, int64_t* __restrict__ confmat,
    int32_t* __restrict__ status) {
  __shared__ unsigned long long s_cm[MAXC * MAXC];
  __shared__ int64_t s_ptr[STAGE];
  if (confmat) {
    for (int i = threadIdx.x; i < C * C; i += THREADS) s_cm[i] = 0ull;
  }
  // the CSR itself: monotone pointers from 0 to num_points, first-hop indices in range
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x; v < num_clusters; v += stride) {
    if (pointers[v + 1] < pointers[v]) atomicAdd(&status[ST_POINTERS], 1);
    if (idx_a) {
      const int64_t a = idx_a[v];
      if (a < 0 || a >= num_label) atomicAdd(&status[ST_FIRST], 1);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 &&
      (pointers[0] != 0 || pointers[num_clusters] != num_points))
    atomicAdd(&status[ST_POINTERS], 1);

  const int64_t tiles = cdiv(num_points, (int64_t)TILE);
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t base = t * TILE;
    const int64_t end = base + TILE < num_points ? base + TILE : num_points;
    const int64_t v_lo = last_not_above(pointers, (int64_t)0, num_clusters - 1, base);
    const int64_t v_hi = last_not_above(pointers, v_lo, num_clusters - 1, end - 1);
    const int64_t staged = v_hi - v_lo + 2;               // pointers[v_lo .. v_hi + 1]
    const bool in_lds = staged <= STAGE;                  // (not with many empty clusters)
    __syncthreads();
    if (in_lds)
      for (int k = threadIdx.x; k < (int)staged; k += THREADS) s_ptr[k] = pointers[v_lo + k];
    __syncthreads();
    for (int64_t j = base + threadIdx.x; j < end; j += THREADS) {
      int64_t v, first, last;
      if (in_lds) {
        const int64_t k = last_not_above(s_ptr, (int64_t)0, staged - 2, j);
        v = v_lo + k;
        first = s_ptr[k];
        last = s_ptr[k + 1];
      } else {
        v = last_not_above(pointers, v_lo, v_hi, j);
        first = pointers[v];
        last = pointers[v + 1];
      }
      if (!(first <= j && j < last)) continue;             // position of no cluster (counted above)
      const int64_t q = points[j];
      if (q < 0 || q >= num_points) {
        atomicAdd(&status[ST_SECOND], 1);
        continue;
      }
      const int64_t a = idx_a ? idx_a[v] : v;
      const int64_t val = a >= 0 && a < num_label ? label[a] : -1;
      if (out) out[q] = val;
      if (confmat) tally(s_cm, C, target[q], val);
    }
  }
  if (confmat) flush(s_cm, C, confmat);
}

inline bool size_ok(int64_t n) { return n >= 0; }

}  // namespace
}  // namespace spt

using namespace spt;

extern "C" int spt_row_argmax_f32(const float* logits, int64_t rows, int C, const int64_t* hist,
                                  int ncols, int64_t* pred, uint8_t* is_void,
                                  spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(size_ok(rows), "negative row count");
  SPT_CHECK_ARG((hist != nullptr) == (is_void != nullptr), "hist and is_void come together");
  SPT_CHECK_ARG(pred || hist, "nothing to compute: pred and the hist / is_void pair are null");
  SPT_CHECK_ARG(!pred || (logits && C >= 1), "pred needs logits with C >= 1");
  SPT_CHECK_ARG(!hist || ncols >= 1, "hist needs ncols >= 1");
  if (rows == 0) return 0;
  row_argmax_kernel<<<stream_grid(rows, THREADS), THREADS, 0, stream>>>(logits, rows, C, hist,
                                                                        ncols, pred, is_void);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_rows_accumulate_f32(float* acc, int64_t N, const float* src,
                                       const int64_t* node_id, int64_t n, int C, int32_t* stamp,
                                       int run, int32_t* status, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(size_ok(N) && size_ok(n), "negative size");
  SPT_CHECK_ARG(C >= 1, "C >= 1");
  SPT_CHECK_ARG(run >= 1, "run >= 1 (0 is the stamp of a row never written)");
  SPT_CHECK_ARG(acc && src && node_id && stamp && status, "null pointer");
  if (n == 0) return 0;
  rows_accumulate_kernel<<<stream_grid(n, THREADS / ACC_LANES), THREADS, 0, stream>>>(
      acc, N, src, node_id, n, C, stamp, run, status);
  SPT_CHECK_LAUNCH();
  return 0;
}

static int check_confmat(const char* who, const int64_t* target, int C, const int64_t* confmat) {
  if ((target != nullptr) != (confmat != nullptr))
    return fail(-1, "%s: target and confmat come together", who);
  if (confmat && (C < 1 || C > MAXC)) return fail(-1, "%s: 1 <= C <= 32", who);
  return 0;
}

extern "C" int spt_labels_by_index_i64(const int64_t* label, int64_t num_label,
                                       const int64_t* idx_a, int64_t n_a, const int64_t* idx_b,
                                       int64_t n_b, int64_t* out_a, int64_t* out_b,
                                       const int64_t* target, int C, int64_t* confmat,
                                       int32_t* status, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(size_ok(num_label) && size_ok(n_a) && size_ok(n_b), "negative size");
  SPT_CHECK_ARG(label && idx_a && status, "null pointer");
  SPT_CHECK_ARG(idx_b || (n_b == 0 && !out_b), "out_b and n_b need idx_b");
  SPT_CHECK_ARG(out_a || out_b || confmat, "nothing to compute: both outputs and confmat are null");
  if (int st = check_confmat(__func__, target, C, confmat)) return st;
  const int64_t n = idx_b && n_b > n_a ? n_b : n_a;
  if (n == 0) return 0;
  // with a confusion matrix: few, long-lived workgroups, each flushes up to C * C cells
  const int grid = confmat ? (int)std::min<int64_t>(ceil_div(n, (int64_t)THREADS), 1024)
                           : stream_grid(n, THREADS);
  labels_by_index_kernel<<<grid, THREADS, 0, stream>>>(label, num_label, idx_a, n_a, idx_b, n_b,
                                                       out_a, out_b, target, C, confmat, status);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_labels_by_cluster_i64(const int64_t* label, int64_t num_label,
                                         const int64_t* idx_a, const int64_t* pointers,
                                         const int64_t* points, int64_t num_clusters,
                                         int64_t num_points, int64_t* out, const int64_t* target,
                                         int C, int64_t* confmat, int32_t* status,
                                         spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(size_ok(num_label) && size_ok(num_clusters) && size_ok(num_points),
                "negative size");
  SPT_CHECK_ARG(label && pointers && points && status, "null pointer");
  SPT_CHECK_ARG(out || confmat, "nothing to compute: out and confmat are null");
  if (int st = check_confmat(__func__, target, C, confmat)) return st;
  if (num_points == 0 || num_clusters == 0) return 0;
  const int64_t tiles = ceil_div(num_points, (int64_t)TILE);
  const int grid = (int)std::min<int64_t>(tiles, confmat ? 1024 : 256 * 16);
  labels_by_cluster_kernel<<<grid, THREADS, 0, stream>>>(label, num_label, idx_a, pointers, points,
                                                         num_clusters, num_points, out, target, C,
                                                         confmat, status);
  SPT_CHECK_LAUNCH();
  return 0;
}
