// Greedy contour-prior partition: the kernels of one merge round.
//
// Stands where the reference calls torch_graph_components (src/utils/components.py:11-130,
// src/transforms/partition.py:383-653): a greedy agglomeration on the energy
//
//   sum_i s_i |x_i - mean(component of i)|^2 + reg * sum_{cut edges} w
//
// from singletons, every component below min_size merged away.  The rounds are specified in
// DESIGN 7.22; tests/greedy_partition_reference.py restates them in f64 numpy and the kernels
// agree with it label for label and bit for bit.
//
//   spt_component_graph_f32   quotient of an edge list under a relabelling: pairs ordered
//                             lo < hi, self loops dropped, the runs of equal (lo, hi) by the
//                             wide-key sort of sorted_runs.hpp (dropped edges in its tail),
//                             duplicate weights reduced in input order
//   spt_merge_means_f64       m_c = F_c / s_c
//   spt_merge_choose_f64      one lane per edge: gain of the merge, 64-bit atomic min of
//                             (orderable gain << 32 | partner) at both ends
//   spt_merge_resolve         activity, parents, mutual pairs rooted at the smaller id
//   spt_merge_jump            parent <- parent[parent], "something moved" flag
//   spt_merge_accumulate_f64  sizes, feature sums and position sums of the merged components:
//                             members grouped by the stable CSR build, summed in ascending id
//   spt_edge_weights_f32      edge lengths in the rows of pos or x, and their f64 sum
//
// Nothing here adds floats atomically: every float result is a function of the input alone.
// Sums over more than LONG_RUN members are 64 strided partial sums (lane l takes members
// l, l + 64, ...) combined by the fixed xor tree, like the per-voxel means of voxel.hip; shorter
// ones are serial.
// The build sets -ffp-contract=off and no fma is written: a * b + c rounds twice, as numpy does.
#include "sorted_runs.hpp"

namespace spt {
namespace merge {

constexpr int THREADS = 256;
constexpr int LONG_RUN = 512;
constexpr int MAX_COLS = 4096;

enum { RED_ADD = 0, RED_MEAN = 1, RED_MAX = 2, RED_MIN = 3, RED_MUL = 4 };

__device__ __forceinline__ float combine(int reduce, float a, float b) {
  switch (reduce) {
    case RED_MAX: return b > a ? b : a;
    case RED_MIN: return b < a ? b : a;
    case RED_MUL: return a * b;
    default: return a + b;                                    // add, mean
  }
}

// f32 bits whose unsigned order is the order of the floats (-0.0 counts as +0.0)
__device__ __forceinline__ uint32_t orderable_bits(float g) {
  const uint32_t u = __float_as_uint(g + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_orderable_bits(uint32_t b) {
  return __uint_as_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b);
}

constexpr uint64_t NO_CHOICE = ~0ull;

// ---- component graph -------------------------------------------------------------------------
// klo / khi [E]: the ordered pair of every edge, or (C, C) for an edge that is dropped (a self
// loop after relabelling, or an end point out of range - those are counted in *bad).
__global__ __launch_bounds__(THREADS) void key_kernel(
    const int64_t* __restrict__ edge_index, int64_t E, int64_t stride,
    const int64_t* __restrict__ index, int64_t num_src, int64_t C, uint32_t* __restrict__ klo,
    uint32_t* __restrict__ khi, int64_t* __restrict__ bad) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += step) {
    int64_t a = edge_index[e], b = edge_index[stride + e];
    bool ok = a >= 0 && a < num_src && b >= 0 && b < num_src;
    if (ok && index) {
      a = index[a];
      b = index[b];
    }
    ok = ok && a >= 0 && a < C && b >= 0 && b < C;
    if (!ok) atomicAdd((unsigned long long*)bad, 1ull);
    uint32_t lo = (uint32_t)C, hi = (uint32_t)C;
    if (ok && a != b) {
      lo = (uint32_t)(a < b ? a : b);
      hi = (uint32_t)(a < b ? b : a);
    }
    klo[e] = lo;
    khi[e] = hi;
  }
}

// The runs of equal (lo, hi) among the kept edges come from csrc/sorted_runs.hpp: lo is the major
// word, hi the minor one, C the limit that sends the dropped edges to the tail.  keys.major is
// lo in sorted order, keys.minor[keys.order[i]] the hi of sorted position i; starts [R + 1] ends
// with the number of kept edges.  One lane per run; a run longer than LONG_RUN is taken by the
// whole wave afterwards.  *count = R.
__global__ __launch_bounds__(THREADS) void run_reduce_kernel(
    SortedKeys keys, const int32_t* __restrict__ starts, const uint32_t* __restrict__ num_runs,
    const float* __restrict__ w, int reduce, int64_t* __restrict__ out_edges, int64_t out_stride,
    float* __restrict__ out_w, int64_t* __restrict__ count) {
  const uint32_t* __restrict__ perm = keys.order;
  const int lane = threadIdx.x & 63;
  const int64_t R = *num_runs;
  if (blockIdx.x == 0 && threadIdx.x == 0) count[0] = R;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < R;
       base += step) {                                        // wave-uniform trip count
    const int64_t r = base + lane;
    int64_t b = 0, e = 0;
    if (r < R) {
      b = starts[r];
      e = starts[r + 1];
      out_edges[r] = (int64_t)keys.major[b];
      out_edges[out_stride + r] = (int64_t)keys.minor[perm[b]];
    }
    const bool longrun = e - b > LONG_RUN;
    if (r < R && !longrun) {
      float s = w ? w[perm[b]] : 1.0f;
      for (int64_t j = b + 1; j < e; ++j) s = combine(reduce, s, w ? w[perm[j]] : 1.0f);
      if (reduce == RED_MEAN) s = s / (float)(e - b);
      out_w[r] = s;
    }
    uint64_t todo = __ballot(longrun);
    while (todo) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const int64_t b2 = __shfl(b, src, 64), e2 = __shfl(e, src, 64);
      float s = w ? w[perm[b2 + lane]] : 1.0f;                // e2 - b2 > 512: every lane has one
      for (int64_t j = b2 + lane + 64; j < e2; j += 64)
        s = combine(reduce, s, w ? w[perm[j]] : 1.0f);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s = combine(reduce, s, __shfl_xor(s, o, 64));  // fixed tree
      if (reduce == RED_MEAN) s = s / (float)(e2 - b2);
      if (lane == 0) out_w[base + src] = s;
    }
  }
}

// The whole scratch is the shared plan; its size does not depend on the bits, which the entry
// knows only with C (the run starts lie over the unsorted lo word there).
static RunsPlan graph_plan(int64_t E, int bits) { return runs_plan(E, bits, bits, true); }

// ---- round -----------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void means_kernel(
    const double* __restrict__ feat, const int64_t* __restrict__ size, int64_t C, int D,
    double* __restrict__ mean) {
  const int64_t total = C * D;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step)
    mean[t] = feat[t] / (double)size[t / D];
}

// Edges arrive sorted by (lo, hi): neighbouring lanes share their lo row, the hi rows are the
// gather.  The key's value does not depend on the order of the atomics; the plain look first
// spares the memory side most of them.
__device__ __forceinline__ void offer(uint64_t* slot, uint64_t key) {
  const uint64_t seen = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (key < seen) atomicMin((unsigned long long*)slot, (unsigned long long)key);
}

__global__ __launch_bounds__(THREADS) void choose_kernel(
    const double* __restrict__ mean, const int64_t* __restrict__ size, int64_t C, int D,
    const int64_t* __restrict__ edges, int64_t E, int64_t stride, const float* __restrict__ w,
    double reg, uint64_t* __restrict__ best, float* __restrict__ gain) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += step) {
    const int64_t a = edges[e], b = edges[stride + e];
    if (a < 0 || a >= C || b < 0 || b >= C || a == b) {       // not a component graph: no offer
      if (gain) gain[e] = 0.0f;
      continue;
    }
    const double* ma = mean + a * D;
    const double* mb = mean + b * D;
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) {
      const double t = ma[d] - mb[d];
      d2 = d2 + t * t;
    }
    const double sa = (double)size[a], sb = (double)size[b];
    const double delta = ((sa * sb) / (sa + sb)) * d2 - reg * (double)w[e];
    const float g = (float)delta;
    if (gain) gain[e] = g;
    const uint64_t ob = (uint64_t)orderable_bits(g) << 32;
    offer(best + a, ob | (uint64_t)(uint32_t)b);
    offer(best + b, ob | (uint64_t)(uint32_t)a);
  }
}

__device__ __forceinline__ bool is_active(uint64_t key, int64_t s, int64_t min_size,
                                          int only_small) {
  if (key == NO_CHOICE) return false;
  if (s < min_size) return true;
  return !only_small && from_orderable_bits((uint32_t)(key >> 32)) < 0.0f;
}

__global__ __launch_bounds__(THREADS) void resolve_kernel(
    const uint64_t* __restrict__ best, const int64_t* __restrict__ size, int64_t C,
    int64_t min_size, int only_small, int64_t* __restrict__ parent, int64_t* __restrict__ active) {
  __shared__ uint32_t sh[THREADS / 64];
  uint32_t mine = 0;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < C; a += step) {
    const uint64_t ka = best[a];
    int64_t p = a;
    if (is_active(ka, size[a], min_size, only_small)) {
      ++mine;
      const int64_t b = (int64_t)(uint32_t)ka;
      p = b;
      if (a < b && b < C) {                                   // a mutual pair keeps its smaller id
        const uint64_t kb = best[b];
        if ((int64_t)(uint32_t)kb == a && is_active(kb, size[b], min_size, only_small)) p = a;
      }
    }
    parent[a] = p;
  }
  mine = wave_reduce_sum(mine);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = sh[0] + sh[1] + sh[2] + sh[3];
    if (t) atomicAdd((unsigned long long*)active, (unsigned long long)t);    // integer: exact
  }
}

__global__ __launch_bounds__(THREADS) void jump_kernel(
    const int64_t* __restrict__ in, int64_t C, int64_t* __restrict__ out,
    int64_t* __restrict__ changed) {
  bool moved = false;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < C; a += step) {
    int64_t p = in[a];
    if (p < 0 || p >= C) p = a;
    int64_t q = in[p];
    if (q < 0 || q >= C) q = p;
    out[a] = q;
    moved = moved || q != p;
  }
  if (changed && __ballot(moved) && (threadIdx.x & 63) == 0) *changed = 1;
}

// ---- accumulate --------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void sum_sizes_kernel(
    const int64_t* __restrict__ size, const int32_t* __restrict__ perm,
    const int32_t* __restrict__ rowptr, int64_t num_new, int64_t* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < num_new; c += step) {
    int64_t s = 0;
    for (int64_t j = rowptr[c]; j < rowptr[c + 1]; ++j) s += size[perm[j]];
    out[c] = s;
  }
}

// One lane per (new component, column); members in ascending old id (the CSR build is stable).
__global__ __launch_bounds__(THREADS) void sum_rows_kernel(
    const double* __restrict__ x, int cols, const int32_t* __restrict__ perm,
    const int32_t* __restrict__ rowptr, int64_t num_new, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t total = num_new * cols;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < total;
       base += step) {                                        // wave-uniform trip count
    const int64_t t = base + lane;
    int64_t b = 0, e = 0;
    int c = 0;
    if (t < total) {
      const int64_t v = t / cols;
      c = (int)(t - v * cols);
      b = rowptr[v];
      e = rowptr[v + 1];
    }
    const bool longrun = e - b > LONG_RUN;
    if (t < total && !longrun) {
      double s = 0.0;
      for (int64_t j = b; j < e; ++j) s = s + x[(int64_t)perm[j] * cols + c];
      out[t] = s;
    }
    uint64_t todo = __ballot(longrun);
    while (todo) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const int64_t b2 = __shfl(b, src, 64), e2 = __shfl(e, src, 64);
      const int c2 = __shfl(c, src, 64);
      double s = 0.0;
      for (int64_t j = b2 + lane; j < e2; j += 64) s = s + x[(int64_t)perm[j] * cols + c2];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);   // fixed tree
      if (lane == 0) out[base + src] = s;
    }
  }
}

struct AccPlan {
  size_t off_perm, off_rowptr, off_csr, total;
};

static AccPlan acc_plan(int64_t num_old, int64_t num_new) {
  AccPlan p;
  size_t o = 0;
  p.off_perm = o;   o += align_up((size_t)(num_old > 0 ? num_old : 1) * 4, 256);
  p.off_rowptr = o; o += align_up((size_t)(num_new + 1) * 4, 256);
  p.off_csr = o;    o += align_up(spt_csr_build_workspace_bytes(num_old, num_new > 0 ? num_new : 1), 256);
  p.total = o;
  return p;
}

// ---- edge lengths ----------------------------------------------------------------------------
// block sum in a fixed order: lanes by butterfly, then the four waves in sequence
__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = wave_reduce_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

static int length_grid(int64_t E) {
  int64_t b = ceil_div(E > 0 ? E : 1, THREADS);
  if (b > 1024) b = 1024;
  return (int)b;
}

// Lane i of workgroup b takes edges b * 256 + i, + grid * 256, ...: the partial of a workgroup,
// and with it the sum, is a function of E alone.
__global__ __launch_bounds__(THREADS) void lengths_kernel(
    const float* __restrict__ x, int cols, int64_t ld, int64_t n,
    const int64_t* __restrict__ edges, int64_t E, int64_t stride, float* __restrict__ dist,
    double* __restrict__ part, int64_t* __restrict__ bad) {
  __shared__ double sh[THREADS / 64];
  double sum = 0.0;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += step) {
    const int64_t a = edges[e], b = edges[stride + e];
    float len = 0.0f;
    if (a < 0 || a >= n || b < 0 || b >= n) {
      atomicAdd((unsigned long long*)bad, 1ull);
    } else {
      double d2 = 0.0;
      for (int c = 0; c < cols; ++c) {
        const double t = (double)x[a * ld + c] - (double)x[b * ld + c];
        d2 = d2 + t * t;
      }
      len = (float)sqrt(d2);
    }
    dist[e] = len;
    sum = sum + (double)len;
  }
  const double bs = block_sum(sum, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = bs;
}

__global__ __launch_bounds__(THREADS) void finish_sum_kernel(
    const double* __restrict__ part, int nblocks, double* __restrict__ out) {
  __shared__ double sh[THREADS / 64];
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += THREADS) s = s + part[b];
  const double t = block_sum(s, sh);
  if (threadIdx.x == 0) out[0] = t;
}

}  // namespace merge
}  // namespace spt

using namespace spt;
using namespace spt::merge;

extern "C" size_t spt_component_graph_workspace_bytes(int64_t num_edges) {
  if (num_edges < 0) return 0;
  return graph_plan(num_edges, 1).total;
}

extern "C" int spt_component_graph_f32(const int64_t* edge_index, int64_t num_edges,
                                       int64_t edge_stride, const float* edge_attr,
                                       const int64_t* index, int64_t num_nodes,
                                       int64_t num_components, int reduce, int64_t* out_edges,
                                       int64_t out_stride, float* out_attr, int64_t* counts,
                                       void* ws, size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t E = num_edges, C = num_components;
  SPT_CHECK_ARG(E >= 0 && E < ((int64_t)1 << 31) - SORT_TILE, "num_edges out of range");
  SPT_CHECK_ARG(num_nodes >= 0 && C >= 0 && C < ((int64_t)1 << 31) && num_nodes < ((int64_t)1 << 31),
                "node counts out of range (< 2^31)");
  SPT_CHECK_ARG(index || C == num_nodes, "without an index the components are the nodes");
  SPT_CHECK_ARG(reduce >= RED_ADD && reduce <= RED_MUL, "reduce: 0 add, 1 mean, 2 max, 3 min, 4 mul");
  SPT_CHECK_ARG(edge_stride >= E && out_stride >= E, "row strides shorter than the rows");
  SPT_CHECK_ARG(counts != nullptr, "counts is null");
  (void)hipMemsetAsync(counts, 0, 2 * 8, stream);
  if (E == 0) return 0;
  SPT_CHECK_ARG(edge_index && out_edges && out_attr, "null pointer");
  const RunsPlan p = graph_plan(E, bits_for(C + 1));
  SPT_CHECK_ARG(ws && ws_bytes >= p.total, "workspace too small");
  char* base = (char*)ws;
  Runs r = runs_carve(base, p, E);

  const int g = stream_grid(E + 1, THREADS);
  key_kernel<<<g, THREADS, 0, stream>>>(edge_index, E, edge_stride, index, num_nodes, C,
                                        r.in.major, r.in.minor, counts + 1);
  SPT_CHECK_ARG(find_runs(base, p, r, E, (uint64_t)C, stream) == 0,
                "scan partials do not fit their region");
  run_reduce_kernel<<<g, THREADS, 0, stream>>>(r.sorted, r.run_start, r.num_runs, edge_attr,
                                               reduce, out_edges, out_stride, out_attr, counts);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_merge_means_f64(const double* feat, const int64_t* size,
                                   int64_t num_components, int d, double* mean,
                                   spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(num_components >= 0 && d >= 1 && d <= MAX_COLS, "shape out of range");
  if (num_components == 0) return 0;
  SPT_CHECK_ARG(feat && size && mean, "null pointer");
  means_kernel<<<stream_grid(num_components * d, THREADS), THREADS, 0, stream>>>(
      feat, size, num_components, d, mean);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_merge_choose_f64(const double* mean, const int64_t* size,
                                    int64_t num_components, int d, const int64_t* edges,
                                    int64_t num_edges, int64_t edge_stride, const float* weights,
                                    double reg, uint64_t* best, float* gain,
                                    spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t C = num_components, E = num_edges;
  SPT_CHECK_ARG(C >= 0 && C < ((int64_t)1 << 31) && d >= 1 && d <= MAX_COLS, "shape out of range");
  SPT_CHECK_ARG(E >= 0 && edge_stride >= E, "edge rows out of range");
  if (C == 0) return 0;
  SPT_CHECK_ARG(best != nullptr, "best is null");
  (void)hipMemsetAsync(best, 0xFF, (size_t)C * 8, stream);
  if (E == 0) return 0;
  SPT_CHECK_ARG(mean && size && edges && weights, "null pointer");
  choose_kernel<<<stream_grid(E, THREADS), THREADS, 0, stream>>>(mean, size, C, d, edges, E,
                                                                 edge_stride, weights, reg, best,
                                                                 gain);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_merge_resolve(const uint64_t* best, const int64_t* size,
                                 int64_t num_components, int64_t min_size, int merge_only_small,
                                 int64_t* parent, int64_t* active, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(num_components >= 0 && num_components < ((int64_t)1 << 31), "shape out of range");
  SPT_CHECK_ARG(active != nullptr, "active is null");
  (void)hipMemsetAsync(active, 0, 8, stream);
  if (num_components == 0) return 0;
  SPT_CHECK_ARG(best && size && parent, "null pointer");
  resolve_kernel<<<stream_grid(num_components, THREADS), THREADS, 0, stream>>>(
      best, size, num_components, min_size, merge_only_small, parent, active);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_merge_jump(const int64_t* parent, int64_t num_components, int64_t* out,
                              int64_t* changed, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(num_components >= 0, "shape out of range");
  SPT_CHECK_ARG(parent != out || num_components == 0, "in place: a pass reads what it writes");
  if (changed) (void)hipMemsetAsync(changed, 0, 8, stream);
  if (num_components == 0) return 0;
  SPT_CHECK_ARG(parent && out, "null pointer");
  jump_kernel<<<stream_grid(num_components, THREADS), THREADS, 0, stream>>>(parent, num_components,
                                                                           out, changed);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_merge_accumulate_workspace_bytes(int64_t num_old, int64_t num_new) {
  if (num_old < 0 || num_new < 0) return 0;
  return acc_plan(num_old, num_new).total;
}

extern "C" int spt_merge_accumulate_f64(const int64_t* label, int64_t num_old, int64_t num_new,
                                        const int64_t* size, const double* feat, int d,
                                        const double* pos, int64_t* size_out, double* feat_out,
                                        double* pos_out, void* ws, size_t ws_bytes,
                                        spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(num_old >= 0 && num_new >= 0 && num_new <= num_old, "counts out of range");
  SPT_CHECK_ARG(d >= 1 && d <= MAX_COLS, "d out of range");
  SPT_CHECK_ARG((pos == nullptr) == (pos_out == nullptr), "pos and pos_out go together");
  if (num_new == 0) return 0;
  SPT_CHECK_ARG(label && size && feat && size_out && feat_out, "null pointer");
  const AccPlan p = acc_plan(num_old, num_new);
  SPT_CHECK_ARG(ws && ws_bytes >= p.total, "workspace too small");
  int32_t* perm = (int32_t*)((char*)ws + p.off_perm);
  int32_t* rowptr = (int32_t*)((char*)ws + p.off_rowptr);
  const int st = spt_csr_build(label, num_old, num_new, perm, rowptr, (char*)ws + p.off_csr,
                               p.total - p.off_csr, stream_);
  if (st != 0) return st;
  sum_sizes_kernel<<<stream_grid(num_new, THREADS), THREADS, 0, stream>>>(size, perm, rowptr,
                                                                         num_new, size_out);
  sum_rows_kernel<<<stream_grid(num_new * d, THREADS), THREADS, 0, stream>>>(feat, d, perm, rowptr,
                                                                            num_new, feat_out);
  if (pos)
    sum_rows_kernel<<<stream_grid(num_new * 3, THREADS), THREADS, 0, stream>>>(pos, 3, perm, rowptr,
                                                                              num_new, pos_out);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_edge_weights_workspace_bytes(int64_t num_edges) {
  if (num_edges < 0) return 0;
  return align_up((size_t)length_grid(num_edges) * 8, 256);
}

extern "C" int spt_edge_weights_f32(const float* rows, int64_t num_nodes, int cols, int64_t ld,
                                    const int64_t* edge_index, int64_t num_edges,
                                    int64_t edge_stride, float* dist, double* sum,
                                    int64_t* bad, void* ws, size_t ws_bytes,
                                    spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t E = num_edges;
  SPT_CHECK_ARG(num_nodes >= 0 && cols >= 1 && cols <= MAX_COLS && ld >= cols, "shape out of range");
  SPT_CHECK_ARG(E >= 0 && edge_stride >= E, "edge rows out of range");
  SPT_CHECK_ARG(sum && bad, "null pointer");
  (void)hipMemsetAsync(sum, 0, 8, stream);
  (void)hipMemsetAsync(bad, 0, 8, stream);
  if (E == 0) return 0;
  SPT_CHECK_ARG(rows && edge_index && dist, "null pointer");
  SPT_CHECK_ARG(ws && ws_bytes >= spt_edge_weights_workspace_bytes(E), "workspace too small");
  const int g = length_grid(E);
  lengths_kernel<<<g, THREADS, 0, stream>>>(rows, cols, ld, num_nodes, edge_index, E, edge_stride,
                                            dist, (double*)ws, bad);
  finish_sum_kernel<<<1, THREADS, 0, stream>>>((const double*)ws, g, sum);
  SPT_CHECK_LAUNCH();
  return 0;
}
