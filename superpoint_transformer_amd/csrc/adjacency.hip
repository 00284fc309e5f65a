// Input graph of the partition, straight from the kNN table.
//
// Replaces the stretch of the preprocessing chain between the neighbour search and the
// cut-pursuit solver:
//
//   AdjacencyGraph(k, w)._process        src/transforms/graph.py:67-96
//   Data.connect_isolated(k_isolated)    src/data/data.py:481-561, src/utils/graph.py:44-53
//   Data.to_trimmed(reduce)              src/data/data.py:563-586, src/utils/graph.py:466-502
//   forward star of the sorted edges     src/transforms/partition.py:190-196
//
// The reference expands the table to an edge list (repeat_interleave + masks), finds the
// isolated nodes with a unique() over every end point, fits the new edges' weights with
// lstsq on an [E, 2] matrix and removes duplicates with a global sort (coalesce).  The table
// makes the sort unnecessary: edge i -> j sits in row i and its mirror, if any, among the
// first k entries of row j, so "is this pair listed twice" is a k-entry look-up, and grouping
// by the smaller end point is a count, a scan and a fill.
//
//   spt_adjacency_stats       one read of the table: valid entries and the f64 sum of their
//                             distances (-> mean), `linked` flags of every source and target,
//                             the repeated-neighbour check, the number of isolated nodes
//   spt_adjacency_regression  the five f64 sums of the least-squares line weight ~ distance
//   spt_adjacency_count       which entries survive, how many per smaller end point, scan
//   spt_adjacency_fill        scatter into the rows, rank-sort each row, emit
//
// The isolated nodes' new edges are extra rows: row n + q belongs to node iso_index[q] and
// holds iso_nn[q, 0..k_iso).  An isolated node's own table row is empty by definition, so
// "the entries of node j" is its table row if linked[j], its extra row otherwise.
//
// An entry i -> j (j != i) is KEPT iff i < j, or node j does not list i.  Kept entries with
// i < j are row i's own; the others are foreign entries of row j (nobody else emits that pair).
// Every pair is emitted once, so the second pass writes each output slot exactly once and the
// per-row rank sort (end points within a row are distinct) removes the arrival order of the
// foreign entries: the output is bitwise reproducible.
//
// Requires: no node repeated within the first k entries of a row (stats reports it; the
// caller then takes the sort-based route), n < 2^31, fewer than 2^32 table entries.
#include "radix_sort.hpp"

namespace spt {
namespace adj {

constexpr int THREADS = 256;
constexpr int SORT_LANES = 8;       // lanes sharing one output row in the emit kernel
constexpr int MAX_K = 64;           // one bit per column in the keep mask

enum { FLAG_REPEATED = 1, FLAG_RANGE = 2 };
enum { RED_MEAN = 0, RED_ADD = 1, RED_MIN = 2, RED_MAX = 3 };

// graph.py:92-94
__device__ __forceinline__ float edge_weight(float d, float w, float mean) {
  return w > 0.f ? 1.0f / (w + d / mean) : 1.0f;
}

// column of `i` among row[0..len), -1 if absent (rows are short: no early exit, the loads
// stay in flight)
__device__ __forceinline__ int find_in_row(const int64_t* __restrict__ row, int len, int64_t i) {
  int at = -1;
  for (int c = 0; c < len; ++c)
    if (row[c] == i && at < 0) at = c;
  return at;
}

// position of `j` in the ascending list iso_index[0..n_iso), -1 if absent
__device__ __forceinline__ int64_t iso_slot(const int64_t* __restrict__ iso_index, int64_t n_iso,
                                            int64_t j) {
  int64_t lo = 0, hi = n_iso;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (iso_index[mid] < j) lo = mid + 1; else hi = mid;
  }
  return (lo < n_iso && iso_index[lo] == j) ? lo : -1;
}

// block sum in a fixed order: lanes by butterfly, then the four waves in sequence
__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = wave_reduce_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// ---- pass A ------------------------------------------------------------------------------
// part[b * 2 + {0, 1}] = valid entries / sum of their distances seen by workgroup b
template <bool SMALL>
__global__ __launch_bounds__(THREADS) void row_stats_kernel(
    const int64_t* __restrict__ nn, const float* __restrict__ dist, int64_t n, int64_t ld, int k,
    uint8_t* __restrict__ linked, double* __restrict__ part, uint32_t* __restrict__ flags) {
  __shared__ double sh[THREADS / 64];
  double cnt = 0.0, sum = 0.0;
  uint32_t flag = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t* row = nn + i * ld;
    bool any = false;
    if constexpr (SMALL) {                                  // k <= 16: the row lives in registers
      int32_t v[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        v[c] = -1;
        if (c < k) {
          const int64_t j = row[c];
          if (j >= n) flag |= FLAG_RANGE;
          else if (j >= 0) v[c] = (int32_t)j;
        }
      }
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        if (v[c] < 0) continue;
        any = true;
        cnt += 1.0;
        if (dist) sum += (double)dist[i * ld + c];
        linked[v[c]] = 1;
#pragma unroll
        for (int c2 = 0; c2 < c; ++c2)
          if (v[c2] == v[c]) flag |= FLAG_REPEATED;
      }
    } else {
      for (int c = 0; c < k; ++c) {
        const int64_t j = row[c];
        if (j >= n) { flag |= FLAG_RANGE; continue; }
        if (j < 0) continue;
        any = true;
        cnt += 1.0;
        if (dist) sum += (double)dist[i * ld + c];
        linked[j] = 1;
        for (int c2 = 0; c2 < c; ++c2)
          if (row[c2] == j) flag |= FLAG_REPEATED;
      }
    }
    if (any) linked[i] = 1;
  }
  const double bc = block_sum(cnt, sh);
  const double bs = block_sum(sum, sh);
  if (threadIdx.x == 0) {
    part[(int64_t)blockIdx.x * 2 + 0] = bc;
    part[(int64_t)blockIdx.x * 2 + 1] = bs;
  }
  if (flag) atomicOr(flags, flag);
}

__global__ __launch_bounds__(THREADS) void count_isolated_kernel(
    const uint8_t* __restrict__ linked, int64_t n, double* __restrict__ part) {
  __shared__ double sh[THREADS / 64];
  double cnt = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    cnt += linked[i] ? 0.0 : 1.0;
  const double bc = block_sum(cnt, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = bc;
}

// out[q] = sum over b of part[b * width + q], one workgroup, fixed order; q < width <= 4.
// `flags` (nullable) goes to out[width].
__global__ __launch_bounds__(THREADS) void finish_sums_kernel(
    const double* __restrict__ part, int nblocks, int width, const uint32_t* __restrict__ flags,
    double* __restrict__ out) {
  __shared__ double sh[THREADS / 64];
  for (int q = 0; q < width; ++q) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += THREADS) s += part[(int64_t)b * width + q];
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) out[q] = t;
  }
  if (flags && threadIdx.x == 0) out[width] = (double)*flags;
}

// ---- regression sums (data.py:535-545) --------------------------------------------------------
// part[b * 4 + ..] = sum d, sum d^2, sum w, sum d w over the valid entries seen by workgroup b;
// d = |pos_i - pos_j| in f32 like the reference, products and sums in f64
__global__ __launch_bounds__(THREADS) void regression_kernel(
    const int64_t* __restrict__ nn, const float* __restrict__ dist, const float* __restrict__ pos,
    int64_t n, int64_t ld, int k, float w, float mean, double* __restrict__ part) {
  __shared__ double sh[THREADS / 64];
  double sd = 0.0, sdd = 0.0, sw = 0.0, sdw = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float px = pos[i * 3 + 0], py = pos[i * 3 + 1], pz = pos[i * 3 + 2];
    for (int c = 0; c < k; ++c) {
      const int64_t j = nn[i * ld + c];
      if (j < 0 || j >= n) continue;
      const float dx = px - pos[j * 3 + 0], dy = py - pos[j * 3 + 1], dz = pz - pos[j * 3 + 2];
      const double d = (double)sqrtf(dx * dx + dy * dy + dz * dz);
      const double wt = (double)edge_weight(dist ? dist[i * ld + c] : 0.f, w, mean);
      sd += d;
      sdd += d * d;
      sw += wt;
      sdw += d * wt;
    }
  }
  const double a = block_sum(sd, sh), b = block_sum(sdd, sh), c = block_sum(sw, sh),
               e = block_sum(sdw, sh);
  if (threadIdx.x == 0) {
    double* p = part + (int64_t)blockIdx.x * 4;
    p[0] = a; p[1] = b; p[2] = c; p[3] = e;
  }
}

// ---- pass B ------------------------------------------------------------------------------
struct Rows {
  const int64_t* nn;         // [n, ld]
  int64_t n, ld;
  int k;
  const uint8_t* linked;     // [n]
  const int64_t* iso_index;  // [n_iso] ascending
  const int64_t* iso_nn;     // [n_iso, k_iso]
  int64_t n_iso;
  int k_iso;
};

// row r of the extended table: node, entries, length
__device__ __forceinline__ void row_of(const Rows& t, int64_t r, int64_t& i,
                                       const int64_t*& row, int& len) {
  if (r < t.n) { i = r; row = t.nn + r * t.ld; len = t.k; }
  else { i = t.iso_index[r - t.n]; row = t.iso_nn + (r - t.n) * t.k_iso; len = t.k_iso; }
}

// where node j lists node i: column of its table row (extra == false) or of its extra row
// (extra == true, slot = which); -1 if it does not.  A table row is only ever listed by table
// rows (a listed node is linked), an extra row can be listed by extra rows only.
__device__ __forceinline__ int partner_column(const Rows& t, bool from_extra, int64_t j, int64_t i,
                                              int64_t& slot) {
  slot = -1;
  if (!from_extra) return find_in_row(t.nn + j * t.ld, t.k, i);
  if (t.linked[j]) return -1;
  slot = iso_slot(t.iso_index, t.n_iso, j);
  if (slot < 0) return -1;
  return find_in_row(t.iso_nn + slot * t.k_iso, t.k_iso, i);
}

__global__ __launch_bounds__(THREADS) void count_kernel(Rows t, uint64_t* __restrict__ keep,
                                                        uint32_t* __restrict__ counts) {
  const int64_t rows = t.n + t.n_iso;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
    int64_t i;
    const int64_t* row;
    int len;
    row_of(t, r, i, row, len);
    uint64_t mask = 0;
    uint32_t own = 0;
    for (int c = 0; c < len; ++c) {
      const int64_t j = row[c];
      if (j < 0 || j >= t.n || j == i) continue;
      if (i < j) {
        mask |= 1ull << c;
        ++own;
      } else {
        int64_t slot;
        if (partner_column(t, r >= t.n, j, i, slot) < 0) {          // unreciprocated: row j's
          mask |= 1ull << c;
          atomicAdd(&counts[j], 1u);
        }
      }
    }
    if (own) atomicAdd(&counts[i], own);
    keep[r] = mask;
  }
}

// ---- pass C ------------------------------------------------------------------------------
__device__ __forceinline__ float merge(int reduce, float a, float b) {
  switch (reduce) {
    case RED_MEAN: return (a + b) / 2.0f;
    case RED_ADD: return a + b;
    case RED_MIN: return fminf(a, b);
    default: return fmaxf(a, b);
  }
}

__global__ __launch_bounds__(THREADS) void fill_kernel(
    Rows t, const float* __restrict__ dist, const float* __restrict__ iso_w, float w, float mean,
    int reduce, int weighted, const uint64_t* __restrict__ keep,
    const uint32_t* __restrict__ row_start, uint32_t* __restrict__ cursor, int64_t num_edges,
    uint32_t* __restrict__ tmp_hi, float* __restrict__ tmp_w) {
  const int64_t rows = t.n + t.n_iso;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
    const uint64_t mask = keep[r];
    if (!mask) continue;
    int64_t i;
    const int64_t* row;
    int len;
    row_of(t, r, i, row, len);
    const bool extra = r >= t.n;
    uint32_t own = 0;
    for (int c = 0; c < len; ++c) {
      if (!((mask >> c) & 1ull)) continue;
      const int64_t j = row[c];
      float wv = 1.0f;
      if (weighted)
        wv = extra ? iso_w[(r - t.n) * t.k_iso + c]
                   : edge_weight(dist ? dist[i * t.ld + c] : 0.f, w, mean);
      int64_t at;
      uint32_t hi;
      if (i < j) {
        if (weighted) {                                     // the mirror entry, dropped by row j
          int64_t slot;
          const int pc = partner_column(t, extra, j, i, slot);
          if (pc >= 0) {
            const float w2 = extra ? iso_w[slot * t.k_iso + pc]
                                   : edge_weight(dist ? dist[j * t.ld + pc] : 0.f, w, mean);
            wv = merge(reduce, wv, w2);
          }
        }
        at = (int64_t)row_start[i] + own++;                 // own entries from the front
        hi = (uint32_t)j;
      } else {
        const uint32_t q = atomicAdd(&cursor[j], 1u);       // foreign entries from the back
        at = (int64_t)row_start[j + 1] - 1 - (int64_t)q;
        hi = (uint32_t)i;
      }
      if (at >= 0 && at < num_edges) {
        tmp_hi[at] = hi;
        if (weighted) tmp_w[at] = wv;
      }
    }
  }
}

// Each output row is rank-sorted by its larger end point (distinct within a row) straight out
// of the staging arrays: element p goes to row_start + #{q : hi[q] < hi[p]}.  Quadratic in the
// row length, which is k plus the number of unreciprocated listers of the node - a handful for
// a kNN table, but correct for any length; SORT_LANES lanes share a row.
__global__ __launch_bounds__(THREADS) void emit_kernel(
    const uint32_t* __restrict__ row_start, int64_t n, int64_t num_edges,
    const uint32_t* __restrict__ tmp_hi, const float* __restrict__ tmp_w,
    int64_t* __restrict__ edge_index, float* __restrict__ edge_attr,
    int64_t* __restrict__ source_csr) {
  const int g = threadIdx.x & (SORT_LANES - 1);
  const int64_t ngroups = (int64_t)gridDim.x * (THREADS / SORT_LANES);
  for (int64_t i = (int64_t)blockIdx.x * (THREADS / SORT_LANES) + threadIdx.x / SORT_LANES; i <= n;
       i += ngroups) {
    const int64_t s = row_start[i];
    if (g == 0) source_csr[i] = s;
    if (i == n) continue;
    const int64_t e = row_start[i + 1];
    for (int64_t p = s + g; p < e; p += SORT_LANES) {
      const uint32_t h = tmp_hi[p];
      int64_t rank = 0;
      for (int64_t q = s; q < e; ++q) rank += tmp_hi[q] < h ? 1 : 0;
      const int64_t at = s + rank;
      if (at < num_edges) {
        edge_index[at] = i;
        edge_index[num_edges + at] = (int64_t)h;
        if (edge_attr) edge_attr[at] = tmp_w[p];
      }
    }
  }
}

static int reduce_grid(int64_t n) {
  int64_t b = ceil_div(n > 0 ? n : 1, THREADS);
  if (b > 1024) b = 1024;
  return (int)b;
}

static bool shape_ok(int64_t n, int64_t ld, int k) {
  return n >= 0 && n < ((int64_t)1 << 31) && k >= 1 && k <= MAX_K && ld >= k;
}

struct FillPlan {
  size_t off_cursor, off_hi, off_w, total;
};

static FillPlan fill_plan(int64_t n, int64_t num_edges) {
  FillPlan p;
  size_t o = 0;
  const int64_t e = num_edges > 0 ? num_edges : 1;
  p.off_cursor = o; o += align_up((size_t)(n > 0 ? n : 1) * 4, 256);
  p.off_hi = o;     o += align_up((size_t)e * 4, 256);
  p.off_w = o;      o += align_up((size_t)e * 4, 256);
  p.total = o;
  return p;
}

}  // namespace adj
}  // namespace spt

using namespace spt;
using namespace spt::adj;

extern "C" size_t spt_adjacency_stats_workspace_bytes(int64_t num_nodes) {
  if (num_nodes < 0) return 0;
  // per-workgroup partials (up to 4 doubles each) + the flag word
  return align_up((size_t)reduce_grid(num_nodes) * 4 * 8, 256) + 256;
}

extern "C" int spt_adjacency_stats(const int64_t* neighbors, const float* distances,
                                   int64_t num_nodes, int64_t ld, int k, uint8_t* linked,
                                   double* stats, void* ws, size_t ws_bytes,
                                   spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t n = num_nodes;
  SPT_CHECK_ARG(shape_ok(n, ld, k), "shape out of range (n < 2^31, 1 <= k <= 64, k <= ld)");
  SPT_CHECK_ARG(stats != nullptr, "stats is null");
  if (n == 0) {
    (void)hipMemsetAsync(stats, 0, 4 * 8, stream);
    return 0;
  }
  SPT_CHECK_ARG(neighbors && linked, "null pointer");
  SPT_CHECK_ARG(ws && ws_bytes >= spt_adjacency_stats_workspace_bytes(n), "workspace too small");
  const int g = reduce_grid(n);
  double* part = (double*)ws;
  uint32_t* flags = (uint32_t*)((char*)ws + align_up((size_t)g * 4 * 8, 256));
  (void)hipMemsetAsync(linked, 0, (size_t)n, stream);
  (void)hipMemsetAsync(flags, 0, 4, stream);
  if (k <= 16)
    row_stats_kernel<true><<<g, THREADS, 0, stream>>>(neighbors, distances, n, ld, k, linked, part,
                                                      flags);
  else
    row_stats_kernel<false><<<g, THREADS, 0, stream>>>(neighbors, distances, n, ld, k, linked,
                                                       part, flags);
  finish_sums_kernel<<<1, THREADS, 0, stream>>>(part, g, 2, nullptr, stats);
  count_isolated_kernel<<<g, THREADS, 0, stream>>>(linked, n, part);
  finish_sums_kernel<<<1, THREADS, 0, stream>>>(part, g, 1, flags, stats + 2);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_adjacency_regression(const int64_t* neighbors, const float* distances,
                                        const float* pos, int64_t num_nodes, int64_t ld, int k,
                                        float w, float mean, double* sums, void* ws,
                                        size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t n = num_nodes;
  SPT_CHECK_ARG(shape_ok(n, ld, k), "shape out of range (n < 2^31, 1 <= k <= 64, k <= ld)");
  SPT_CHECK_ARG(sums != nullptr, "sums is null");
  SPT_CHECK_ARG(w <= 0.f || distances, "w > 0 needs the distances");
  if (n == 0) {
    (void)hipMemsetAsync(sums, 0, 4 * 8, stream);
    return 0;
  }
  SPT_CHECK_ARG(neighbors && pos, "null pointer");
  SPT_CHECK_ARG(ws && ws_bytes >= spt_adjacency_stats_workspace_bytes(n), "workspace too small");
  const int g = reduce_grid(n);
  regression_kernel<<<g, THREADS, 0, stream>>>(neighbors, distances, pos, n, ld, k, w, mean,
                                               (double*)ws);
  finish_sums_kernel<<<1, THREADS, 0, stream>>>((const double*)ws, g, 4, nullptr, sums);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_adjacency_count_workspace_bytes(int64_t num_nodes) {
  if (num_nodes < 0) return 0;
  return scan_part_bytes(num_nodes + 1);
}

extern "C" int spt_adjacency_count(const int64_t* neighbors, int64_t num_nodes, int64_t ld, int k,
                                   const uint8_t* linked, const int64_t* iso_index,
                                   const int64_t* iso_neighbors, int64_t num_isolated,
                                   int k_isolated, uint64_t* keep, uint32_t* row_start, void* ws,
                                   size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t n = num_nodes, n_iso = num_isolated;
  SPT_CHECK_ARG(shape_ok(n, ld, k), "shape out of range (n < 2^31, 1 <= k <= 64, k <= ld)");
  SPT_CHECK_ARG(n_iso >= 0 && n_iso <= n && k_isolated >= 0 && k_isolated <= MAX_K,
                "isolated rows out of range");
  SPT_CHECK_ARG(n * k + n_iso * k_isolated < ((int64_t)1 << 32), "more than 2^32 - 1 entries");
  SPT_CHECK_ARG(row_start != nullptr, "row_start is null");
  SPT_CHECK_ARG(ws && ws_bytes >= spt_adjacency_count_workspace_bytes(n), "workspace too small");
  (void)hipMemsetAsync(row_start, 0, (size_t)(n + 1) * 4, stream);
  if (n > 0) {
    SPT_CHECK_ARG(neighbors && linked && keep, "null pointer");
    SPT_CHECK_ARG(n_iso == 0 || k_isolated == 0 || (iso_index && iso_neighbors),
                  "isolated rows without their tables");
    Rows t{neighbors, n, ld, k, linked, iso_index, iso_neighbors, k_isolated > 0 ? n_iso : 0,
           k_isolated};
    count_kernel<<<stream_grid(t.n + t.n_iso, THREADS), THREADS, 0, stream>>>(t, keep, row_start);
  }
  SPT_CHECK_ARG(device_exclusive_scan(row_start, n + 1, (uint32_t*)ws,
                                      (int64_t)(ws_bytes / 4), stream) == 0,
                "scan partials do not fit their region");
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_adjacency_fill_workspace_bytes(int64_t num_nodes, int64_t num_edges) {
  if (num_nodes < 0 || num_edges < 0) return 0;
  return fill_plan(num_nodes, num_edges).total;
}

extern "C" int spt_adjacency_fill(const int64_t* neighbors, const float* distances,
                                  int64_t num_nodes, int64_t ld, int k, float w, float mean,
                                  const uint8_t* linked, const int64_t* iso_index,
                                  const int64_t* iso_neighbors, const float* iso_weights,
                                  int64_t num_isolated, int k_isolated, int reduce,
                                  const uint64_t* keep, const uint32_t* row_start,
                                  int64_t num_edges, int64_t* edge_index, float* edge_attr,
                                  int64_t* source_csr, void* ws, size_t ws_bytes,
                                  spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t n = num_nodes, n_iso = num_isolated, E = num_edges;
  SPT_CHECK_ARG(shape_ok(n, ld, k), "shape out of range (n < 2^31, 1 <= k <= 64, k <= ld)");
  SPT_CHECK_ARG(n_iso >= 0 && n_iso <= n && k_isolated >= 0 && k_isolated <= MAX_K,
                "isolated rows out of range");
  SPT_CHECK_ARG(E >= 0 && E <= n * k + n_iso * k_isolated, "num_edges out of range");
  SPT_CHECK_ARG(reduce >= RED_MEAN && reduce <= RED_MAX, "reduce: 0 mean, 1 add, 2 min, 3 max");
  SPT_CHECK_ARG(row_start && source_csr, "null pointer");
  const int weighted = edge_attr != nullptr;
  SPT_CHECK_ARG(!weighted || w <= 0.f || distances, "w > 0 needs the distances");
  const FillPlan p = fill_plan(n, E);
  SPT_CHECK_ARG(ws && ws_bytes >= p.total, "workspace too small");
  uint32_t* cursor = (uint32_t*)((char*)ws + p.off_cursor);
  uint32_t* tmp_hi = (uint32_t*)((char*)ws + p.off_hi);
  float* tmp_w = (float*)((char*)ws + p.off_w);
  if (n > 0 && E > 0) {
    SPT_CHECK_ARG(neighbors && linked && keep && edge_index, "null pointer");
    const bool iso = n_iso > 0 && k_isolated > 0;
    SPT_CHECK_ARG(!iso || (iso_index && iso_neighbors && (!weighted || iso_weights)),
                  "isolated rows without their tables");
    Rows t{neighbors, n, ld, k, linked, iso_index, iso_neighbors, iso ? n_iso : 0, k_isolated};
    (void)hipMemsetAsync(cursor, 0, (size_t)n * 4, stream);
    fill_kernel<<<stream_grid(t.n + t.n_iso, THREADS), THREADS, 0, stream>>>(
        t, distances, iso_weights, w, mean, reduce, weighted, keep, row_start, cursor, E, tmp_hi,
        tmp_w);
  }
  emit_kernel<<<stream_grid(n + 1, THREADS / SORT_LANES), THREADS, 0, stream>>>(
      row_start, n, E, tmp_hi, tmp_w, edge_index, edge_attr, source_csr);
  SPT_CHECK_LAUNCH();
  return 0;
}
