// Superedges in one pass per edge.
//
// Replaces, for the edges whose two segments fit a workgroup, the whole of `subedges`
// (src/utils/graph.py:99-463) and `_minimalistic_horizontal_edge_features`
// (src/transforms/graph.py:950-1060).  The reference - and graph.subedges here - expands every
// edge into the points of both segments and runs ~25 passes, four of them sorts, over those
// edge-wise lists.  Here a workgroup owns an edge: both segments are projected into the edge's
// frame and kept in LDS, filtered, ordered, cut to `st_k` points a side, ordered again along the
// first principal component, paired rank by rank and reduced to the 7 features.  Nothing is
// expanded in memory; per edge 28 bytes (and, on request, its pairs) are written.
//
// Two kernel shapes from one template: a wave per edge for segments of at most 64 points a side
// (one point per lane), 256 threads per edge up to CAP_MED points a side (4 points per thread).
// Sorts are rank sorts in LDS - rank = number of live keys ahead, equal keys in CSR order - which
// is what two stable sorts on (key, group) give.  Every sum is a fixed tree of f64 partials (lane
// stride, wave butterfly, waves in order): two runs are bit-equal, no float atomics anywhere.
#include "geof_core.hpp"
#include "radix_sort.hpp"

namespace spt {
namespace sedge {

constexpr int CAP_SMALL = 64;
constexpr int CAP_MED = 1024;
enum { SW_HALFSPACE = 1, SW_BBOX = 2, SW_FLIP = 4, SW_SOURCE_SORT = 8 };

struct Params {
  const float* pos;
  int64_t num_points;
  const int32_t* perm;
  const int32_t* rowptr;
  int64_t num_segments;
  const int64_t* edges;
  int64_t num_edges, edge_stride;
  const int64_t* anchors;
  const int32_t* list;       // edge ids of this launch
  int64_t list_len;
  float ratio, margin;
  int k_min, switches, count_only;
  float* edge_attr;
  int32_t* count;
  const uint32_t* pair_offset;
  int64_t* pairs;
  int64_t* uid;
  int64_t num_pairs;
};

struct OpSum { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct OpMin { template <typename T> __device__ T operator()(T a, T b) const { return b < a ? b : a; } };
struct OpMax { template <typename T> __device__ T operator()(T a, T b) const { return b > a ? b : a; } };

// every thread of the workgroup gets op over all threads' v[q]; fixed order
template <int NW, int N, typename T, typename F>
__device__ __forceinline__ void block_reduce(T (&v)[N], void* scratch_, F op) {
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[q] = op(v[q], (T)__shfl_xor(v[q], o, 64));
  if constexpr (NW > 1) {
    T* scratch = (T*)scratch_;
    const int w = threadIdx.x >> 6;
    __syncthreads();                                   // scratch reuse across calls
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int q = 0; q < N; ++q) scratch[w * N + q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) {
      T a = scratch[q];
#pragma unroll
      for (int k = 1; k < NW; ++k) a = op(a, scratch[k * N + q]);
      v[q] = a;
    }
  }
}

__device__ __forceinline__ float norm3(const float v[3]) {
  return sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

__device__ __forceinline__ float dot3(const float a[3], const float b[3]) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// graph.base_vectors_3d (src/utils/geometry.py:42-78), rows = axes, both fill-ins
__device__ __forceinline__ void base_vectors(const float x[3], float b[3][3]) {
  float a[3] = {x[0], x[1], x[2]};
  if (norm3(a) == 0.f) { a[0] = 1.f; a[1] = 0.f; a[2] = 0.f; }
  const float na = norm3(a);
#pragma unroll
  for (int q = 0; q < 3; ++q) b[0][q] = a[q] / na;
  float c[3] = {b[0][1] - b[0][2], b[0][2] - b[0][0], b[0][0] - b[0][1]};
  if (norm3(c) == 0.f) { c[0] = 2.f; c[1] = 1.f; c[2] = -1.f; }
  const float nc = norm3(c);
#pragma unroll
  for (int q = 0; q < 3; ++q) b[1][q] = c[q] / nc;
  b[2][0] = b[0][1] * b[1][2] - b[0][2] * b[1][1];
  b[2][1] = b[0][2] * b[1][0] - b[0][0] * b[1][2];
  b[2][2] = b[0][0] * b[1][1] - b[0][1] * b[1][0];
}

__device__ __forceinline__ uint32_t ordered_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int THREADS, int CAP>
__global__ __launch_bounds__(THREADS) void superedge_kernel(const Params p) {
  constexpr int ITEMS = CAP / THREADS, NW = THREADS / 64;
  __shared__ float sx[2][CAP], sy[2][CAP], sz[2][CAP];
  __shared__ int sid[2][CAP];
  __shared__ double scratch[NW * 9];
  const int tid = threadIdx.x;

  for (int64_t b = blockIdx.x; b < p.list_len; b += gridDim.x) {
    __syncthreads();                                   // LDS of the previous edge is done with
    const int64_t e = p.list[b];
    if (e < 0 || e >= p.num_edges) continue;
    // ---- the edge, its segments, its anchors: everything read is checked before it is used
    const int64_t s = p.edges[e], t = p.edges[p.edge_stride + e];
    const int64_t a_s = p.anchors[e], a_t = p.anchors[p.num_edges + e];
    bool ok = s >= 0 && s < p.num_segments && t >= 0 && t < p.num_segments && a_s >= 0 &&
              a_s < p.num_points && a_t >= 0 && a_t < p.num_points;
    int lo[2] = {0, 0}, n[2] = {0, 0};
    if (ok) {
      lo[0] = p.rowptr[s]; n[0] = p.rowptr[s + 1] - lo[0];
      lo[1] = p.rowptr[t]; n[1] = p.rowptr[t + 1] - lo[1];
#pragma unroll
      for (int sd = 0; sd < 2; ++sd)
        ok = ok && lo[sd] >= 0 && n[sd] >= 1 && n[sd] <= CAP && (int64_t)lo[sd] + n[sd] <= p.num_points;
    }
    if (!ok) {                                         // not an edge this kernel can own
      if (tid == 0) {
        p.count[e] = 0;
        if (!p.count_only)
          for (int q = 0; q < 7; ++q) p.edge_attr[e * 7 + q] = 0.f;
      }
      continue;
    }
    float anc[2][3], dir[3], base[3][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      anc[0][q] = p.pos[a_s * 3 + q];
      anc[1][q] = p.pos[a_t * 3 + q];
      dir[q] = anc[1][q] - anc[0][q];
    }
    base_vectors(dir, base);

    // ---- project both segments into the frame, each side about its own anchor
    float px[2][ITEMS], py[2][ITEMS], pz[2][ITEMS];
    int pid[2][ITEMS];
    bool alive[2][ITEMS];
#pragma unroll
    for (int sd = 0; sd < 2; ++sd)
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        const int j = tid + i * THREADS;
        alive[sd][i] = j < n[sd];
        px[sd][i] = py[sd][i] = pz[sd][i] = 0.f;
        pid[sd][i] = 0;
        if (alive[sd][i]) {
          int id = p.perm[lo[sd] + j];
          if (id < 0 || id >= p.num_points) id = 0;
          pid[sd][i] = id;
          float d[3];
#pragma unroll
          for (int q = 0; q < 3; ++q) d[q] = p.pos[(int64_t)id * 3 + q] - anc[sd][q];
          px[sd][i] = dot3(d, base[0]);
          py[sd][i] = dot3(d, base[1]);
          pz[sd][i] = dot3(d, base[2]);
        }
      }
    int size[2] = {n[0], n[1]};

    // a filter never empties a side (idx_preserving_mask)
    auto apply = [&](bool (&m)[2][ITEMS]) {
      int kept[2] = {0, 0};
#pragma unroll
      for (int sd = 0; sd < 2; ++sd)
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) kept[sd] += (alive[sd][i] && m[sd][i]) ? 1 : 0;
      block_reduce<NW>(kept, scratch, OpSum());
#pragma unroll
      for (int sd = 0; sd < 2; ++sd)
        if (kept[sd] > 0) {
          size[sd] = kept[sd];
#pragma unroll
          for (int i = 0; i < ITEMS; ++i) alive[sd][i] = alive[sd][i] && m[sd][i];
        }
    };

    if (p.switches & SW_HALFSPACE) {
      bool m[2][ITEMS];
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        m[0][i] = px[0][i] <= p.margin;
        m[1][i] = px[1][i] >= -p.margin;
      }
      apply(m);
    }
    if (p.switches & SW_BBOX) {
      const float inf = __builtin_huge_valf();
      float mn[4] = {inf, inf, inf, inf}, mx[4] = {-inf, -inf, -inf, -inf};
#pragma unroll
      for (int sd = 0; sd < 2; ++sd)
#pragma unroll
        for (int i = 0; i < ITEMS; ++i)
          if (alive[sd][i]) {
            mn[sd * 2] = fminf(mn[sd * 2], py[sd][i]);
            mn[sd * 2 + 1] = fminf(mn[sd * 2 + 1], pz[sd][i]);
            mx[sd * 2] = fmaxf(mx[sd * 2], py[sd][i]);
            mx[sd * 2 + 1] = fmaxf(mx[sd * 2 + 1], pz[sd][i]);
          }
      block_reduce<NW>(mn, scratch, OpMin());
      block_reduce<NW>(mx, scratch, OpMax());
      float st_min[2], st_max[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        st_min[q] = fminf(fmaxf(mn[q], mn[2 + q]), -p.margin);
        st_max[q] = fmaxf(fminf(mx[q], mx[2 + q]), p.margin);
      }
      bool m[2][ITEMS];
#pragma unroll
      for (int sd = 0; sd < 2; ++sd)
#pragma unroll
        for (int i = 0; i < ITEMS; ++i)
          m[sd][i] = py[sd][i] >= st_min[0] && pz[sd][i] >= st_min[1] &&
                     py[sd][i] <= st_max[0] && pz[sd][i] <= st_max[1];
      apply(m);
    }

    // ---- the same number of points on both sides (graph.py:379-399)
    int st_k;
    {
      int k[2];
#pragma unroll
      for (int sd = 0; sd < 2; ++sd) {
        int64_t v = (int64_t)((float)size[sd] * p.ratio);
        if (v < p.k_min) v = p.k_min;
        if (v > size[sd]) v = size[sd];
        k[sd] = (int)v;
      }
      st_k = k[0] < k[1] ? k[0] : k[1];
    }
    if (p.count_only) {
      if (tid == 0) p.count[e] = st_k;
      continue;
    }

    // ---- order by the first coordinate (source descending, target ascending) and keep st_k
#pragma unroll
    for (int sd = 0; sd < 2; ++sd)
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        const int j = tid + i * THREADS;
        if (j < n[sd]) {
          sx[sd][j] = px[sd][i];
          sid[sd][j] = alive[sd][i] ? 1 : 0;
        }
      }
    __syncthreads();
    int rank[2][ITEMS];
#pragma unroll
    for (int sd = 0; sd < 2; ++sd) {
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) rank[sd][i] = 0;
      for (int j = 0; j < n[sd]; ++j) {
        const float kj = sx[sd][j];
        const bool live = sid[sd][j] != 0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
          const float ki = px[sd][i];
          const bool ahead = sd == 0 ? kj > ki : kj < ki;
          rank[sd][i] += (live && (ahead || (kj == ki && j < tid + i * THREADS))) ? 1 : 0;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int sd = 0; sd < 2; ++sd)
#pragma unroll
      for (int i = 0; i < ITEMS; ++i)
        if (alive[sd][i] && rank[sd][i] < st_k) {
          const int r = rank[sd][i];
          sx[sd][r] = px[sd][i]; sy[sd][r] = py[sd][i]; sz[sd][r] = pz[sd][i];
          sid[sd][r] = pid[sd][i];
        }
    __syncthreads();
    // from here on item i of a thread is the point of rank r = tid + i * THREADS < st_k
#pragma unroll
    for (int sd = 0; sd < 2; ++sd)
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        const int r = tid + i * THREADS;
        alive[sd][i] = r < st_k;
        if (alive[sd][i]) {
          px[sd][i] = sx[sd][r]; py[sd][i] = sy[sd][r]; pz[sd][i] = sz[sd][r];
          pid[sd][i] = sid[sd][r];
        }
      }

    // ---- first principal component of each side (scatter_pca: f64 moments about the first row)
    float pc[2][3], centroid[2][3];
#pragma unroll
    for (int sd = 0; sd < 2; ++sd) {
      const double ox = sx[sd][0], oy = sy[sd][0], oz = sz[sd][0];
      double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < ITEMS; ++i)
        if (alive[sd][i]) {
          const double dx = (double)px[sd][i] - ox, dy = (double)py[sd][i] - oy,
                       dz = (double)pz[sd][i] - oz;
          m[0] += dx; m[1] += dy; m[2] += dz;
          m[3] += dx * dx; m[4] += dx * dy; m[5] += dx * dz;
          m[6] += dy * dy; m[7] += dy * dz; m[8] += dz * dz;
        }
      block_reduce<NW>(m, scratch, OpSum());
      const double inv = 1.0 / (double)st_k;
      const double mx = m[0] * inv, my = m[1] * inv, mz = m[2] * inv;
      double a[3][3], w[3], v[3][3];
      a[0][0] = m[3] * inv - mx * mx;
      a[0][1] = a[1][0] = m[4] * inv - mx * my;
      a[0][2] = a[2][0] = m[5] * inv - mx * mz;
      a[1][1] = m[6] * inv - my * my;
      a[1][2] = a[2][1] = m[7] * inv - my * mz;
      a[2][2] = m[8] * inv - mz * mz;
      eigh3(a, w, v);
#pragma unroll
      for (int q = 0; q < 3; ++q) pc[sd][q] = (float)v[q][2];
      double c[3] = {0, 0, 0};
#pragma unroll
      for (int i = 0; i < ITEMS; ++i)
        if (alive[sd][i]) { c[0] += (double)px[sd][i]; c[1] += (double)py[sd][i]; c[2] += (double)pz[sd][i]; }
      block_reduce<NW>(c, scratch, OpSum());
#pragma unroll
      for (int q = 0; q < 3; ++q) centroid[sd][q] = (float)(c[q] / (double)st_k);
    }

    // ---- direction of the target's ordering (graph.py:437-444)
    if (p.switches & SW_SOURCE_SORT) {
#pragma unroll
      for (int q = 0; q < 3; ++q) pc[1][q] = pc[0][q];
    } else if (p.switches & SW_FLIP) {
      unsigned long long best[1] = {~0ull};
#pragma unroll
      for (int i = 0; i < ITEMS; ++i)
        if (alive[1][i]) {
          const float c[3] = {px[1][i], py[1][i], pz[1][i]};
          const float pr = dot3(c, pc[1]) + 0.f;       // -0 -> +0: equal values tie to the first
          const unsigned long long key =
              ((unsigned long long)ordered_bits(pr) << 32) | (uint32_t)(tid + i * THREADS);
          best[0] = key < best[0] ? key : best[0];
        }
      block_reduce<NW>(best, scratch, OpMin());
      int am = (int)(uint32_t)best[0];
      if (am < 0 || am >= st_k) am = 0;                // NaN projections: any row, like an argmin
      float u[3] = {sx[1][am] - centroid[0][0], sy[1][am] - centroid[0][1], sz[1][am] - centroid[0][2]};
      const float nu = norm3(u);
#pragma unroll
      for (int q = 0; q < 3; ++q) u[q] = u[q] / nu;
      if (dot3(pc[0], pc[1]) <= dot3(pc[0], u)) {
#pragma unroll
        for (int q = 0; q < 3; ++q) pc[1][q] = -pc[1][q];
      }
    }

    // ---- order each side along its component about its own centroid (sparse.py:107-137)
    __syncthreads();                                   // sx[1][am] has been read by everyone
#pragma unroll
    for (int sd = 0; sd < 2; ++sd)
#pragma unroll
      for (int i = 0; i < ITEMS; ++i)
        if (alive[sd][i]) {
          const float d[3] = {px[sd][i] - centroid[sd][0], py[sd][i] - centroid[sd][1],
                              pz[sd][i] - centroid[sd][2]};
          px[sd][i] = dot3(d, pc[sd]);
          sx[sd][tid + i * THREADS] = px[sd][i];
        }
    __syncthreads();
#pragma unroll
    for (int sd = 0; sd < 2; ++sd) {
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) rank[sd][i] = 0;
      for (int j = 0; j < st_k; ++j) {
        const float kj = sx[sd][j];
#pragma unroll
        for (int i = 0; i < ITEMS; ++i)
          rank[sd][i] += (kj < px[sd][i] || (kj == px[sd][i] && j < tid + i * THREADS)) ? 1 : 0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int sd = 0; sd < 2; ++sd)
#pragma unroll
      for (int i = 0; i < ITEMS; ++i)
        if (alive[sd][i] && rank[sd][i] < st_k) sid[sd][rank[sd][i]] = pid[sd][i];
    __syncthreads();

    // ---- pairs rank by rank, and the 7 features of the edge from them
    float off[ITEMS][3];
    double sums[4] = {0, 0, 0, 0};
    const int64_t first = p.pair_offset ? (int64_t)p.pair_offset[e] : 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      const int r = tid + i * THREADS;
      off[i][0] = off[i][1] = off[i][2] = 0.f;
      if (r < st_k) {
        int a = sid[0][r], c = sid[1][r];
        if (a < 0 || a >= p.num_points) a = 0;           // NaN keys leave ranks unassigned
        if (c < 0 || c >= p.num_points) c = 0;
        if (p.pair_offset && first + r < p.num_pairs) {
          p.pairs[first + r] = a;
          p.pairs[p.num_pairs + first + r] = c;
          p.uid[first + r] = e;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) off[i][q] = p.pos[(int64_t)c * 3 + q] - p.pos[(int64_t)a * 3 + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) sums[q] += (double)off[i][q];
        sums[3] += (double)norm3(off[i]);
      }
    }
    block_reduce<NW>(sums, scratch, OpSum());
    float mean_off[3], fb[3][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) mean_off[q] = (float)(sums[q] / (double)st_k);
    const float mean_dist = (float)sqrt(sums[3] / (double)st_k);    // one rounding
    base_vectors(mean_off, fb);
    double us[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < ITEMS; ++i)
      if (tid + i * THREADS < st_k) {
        const float u0 = dot3(off[i], fb[0]), u1 = dot3(off[i], fb[1]), u2 = dot3(off[i], fb[2]);
        off[i][0] = u0; off[i][1] = u1; off[i][2] = u2;
        us[0] += (double)u0; us[1] += (double)u1; us[2] += (double)u2;
      }
    block_reduce<NW>(us, scratch, OpSum());
    double dv[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < ITEMS; ++i)
      if (tid + i * THREADS < st_k) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float d = off[i][q] - (float)(us[q] / (double)st_k);
          dv[q] += (double)(d * d);
        }
      }
    block_reduce<NW>(dv, scratch, OpSum());
    if (tid == 0) {
      // torch_scatter's scatter_std as segment_std_kernel computes it (unbiased, clamped + 1e-6)
      const float denom = (float)((st_k - 1 > 1) ? (st_k - 1) : 1) + 1e-6f;
      float* out = p.edge_attr + e * 7;
#pragma unroll
      for (int q = 0; q < 3; ++q) out[q] = mean_off[q];
#pragma unroll
      for (int q = 0; q < 3; ++q)
        out[3 + q] = fminf(fmaxf((float)sqrt(dv[q] / (double)denom), -2.f), 2.f);
      out[6] = mean_dist;
      p.count[e] = st_k;
    }
  }
}

// class of every edge from the sizes of its two segments: 0 small, 1 medium, 2 large (or not
// an edge of this graph: the composition refuses it with a message)
__global__ void class_flags_kernel(const int32_t* __restrict__ rowptr, int64_t num_segments,
                                   const int64_t* __restrict__ edges, int64_t E,
                                   int64_t edge_stride, uint32_t* __restrict__ f0,
                                   uint32_t* __restrict__ f1, uint32_t* __restrict__ f2) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= E; e += stride) {
    int c = 3;                                          // slot E: the totals land here
    if (e < E) {
      const int64_t s = edges[e], t = edges[edge_stride + e];
      c = 2;
      if (s >= 0 && s < num_segments && t >= 0 && t < num_segments) {
        const int ns = rowptr[s + 1] - rowptr[s], nt = rowptr[t + 1] - rowptr[t];
        const int m = ns > nt ? ns : nt, l = ns < nt ? ns : nt;
        if (l >= 1 && m <= CAP_SMALL) c = 0;
        else if (l >= 1 && m <= CAP_MED) c = 1;
      }
    }
    f0[e] = c == 0; f1[e] = c == 1; f2[e] = c == 2;
  }
}

__global__ void class_lists_kernel(const uint32_t* __restrict__ f0, const uint32_t* __restrict__ f1,
                                   const uint32_t* __restrict__ f2, int64_t E,
                                   int32_t* __restrict__ order, int64_t* __restrict__ counts) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n0 = f0[E], n1 = f1[E];
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += stride) {
    if (e == 0) { counts[0] = n0; counts[1] = n1; counts[2] = f2[E]; }
    int64_t dst;
    if (f0[e + 1] != f0[e]) dst = f0[e];
    else if (f1[e + 1] != f1[e]) dst = n0 + f1[e];
    else dst = n0 + n1 + f2[e];
    if (dst >= 0 && dst < E) order[dst] = (int32_t)e;
  }
}

__global__ void count_copy_kernel(const int32_t* __restrict__ count, int64_t E,
                                  uint32_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= E; e += stride)
    out[e] = e < E ? (uint32_t)(count[e] > 0 ? count[e] : 0) : 0u;
}

struct Plan {
  size_t off_f[3], off_part, total;
  int64_t part_cap;
};

static Plan make_plan(int64_t E) {
  Plan p;
  size_t o = 0;
  const int64_t m = (E > 0 ? E : 0) + 1;
  for (int q = 0; q < 3; ++q) { p.off_f[q] = o; o += align_up((size_t)m * 4, 256); }
  p.off_part = o; o += scan_part_bytes(m);
  p.part_cap = (int64_t)((o - p.off_part) / 4);
  p.total = o;
  return p;
}

}  // namespace sedge
}  // namespace spt

using namespace spt;
using namespace spt::sedge;

static const int64_t SEDGE_MAX = ((int64_t)1 << 31) - 1;

extern "C" int spt_superedge_capacity(void) { return CAP_MED; }

extern "C" size_t spt_superedge_workspace_bytes(int64_t num_edges) {
  if (num_edges < 0) return 0;
  return make_plan(num_edges).total;
}

extern "C" int spt_superedge_classify(const int32_t* rowptr, int64_t num_segments,
                                      const int64_t* edges, int64_t num_edges,
                                      int64_t edge_stride, int32_t* order, int64_t* counts,
                                      void* ws, size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t E = num_edges;
  SPT_CHECK_ARG(E >= 0 && E < SEDGE_MAX - SCAN_TILE && num_segments >= 0 && num_segments < SEDGE_MAX &&
                edge_stride >= E, "shape out of range");
  SPT_CHECK_ARG(counts != nullptr, "counts is null");
  if (E == 0) {
    (void)hipMemsetAsync(counts, 0, 24, stream);
    return 0;
  }
  SPT_CHECK_ARG(rowptr && edges && order, "null pointer");
  const Plan p = make_plan(E);
  SPT_CHECK_ARG(ws && ws_bytes >= p.total, "workspace too small");
  uint32_t* f[3];
  for (int q = 0; q < 3; ++q) f[q] = (uint32_t*)((char*)ws + p.off_f[q]);
  uint32_t* part = (uint32_t*)((char*)ws + p.off_part);
  const int g = stream_grid(E + 1, 256);
  class_flags_kernel<<<g, 256, 0, stream>>>(rowptr, num_segments, edges, E, edge_stride, f[0],
                                            f[1], f[2]);
  for (int q = 0; q < 3; ++q)
    SPT_CHECK_ARG(device_exclusive_scan(f[q], E + 1, part, p.part_cap, stream) == 0,
                  "scan partials do not fit their region");
  class_lists_kernel<<<g, 256, 0, stream>>>(f[0], f[1], f[2], E, order, counts);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_superedge_pair_offsets(const int32_t* count, int64_t num_edges,
                                          uint32_t* offsets, void* ws, size_t ws_bytes,
                                          spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t E = num_edges;
  SPT_CHECK_ARG(E >= 0 && E < SEDGE_MAX - SCAN_TILE, "shape out of range");
  SPT_CHECK_ARG(offsets != nullptr, "offsets is null");
  SPT_CHECK_ARG(E == 0 || count, "null pointer");
  const int64_t cap = ws ? (int64_t)(ws_bytes / 4) : 0;
  SPT_CHECK_ARG(cap >= scan_part_entries(E + 1), "workspace too small");
  count_copy_kernel<<<stream_grid(E + 1, 256), 256, 0, stream>>>(count, E, offsets);
  SPT_CHECK_ARG(device_exclusive_scan(offsets, E + 1, (uint32_t*)ws, cap, stream) == 0,
                "scan partials do not fit their region");
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_superedge_f32(const float* pos, int64_t num_points, const int32_t* perm,
                                 const int32_t* rowptr, int64_t num_segments,
                                 const int64_t* edges, int64_t num_edges, int64_t edge_stride,
                                 const int64_t* anchors, const int32_t* order, int64_t num_small,
                                 int64_t num_medium, float ratio, int k_min, float margin,
                                 int switches, int count_only, float* edge_attr, int32_t* count,
                                 const uint32_t* pair_offset, int64_t* pairs, int64_t* uid,
                                 int64_t num_pairs, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(num_points >= 0 && num_points <= SEDGE_MAX, "more than 2^31 - 1 points");
  SPT_CHECK_ARG(num_edges >= 0 && num_edges < SEDGE_MAX && num_segments >= 0 &&
                num_segments < SEDGE_MAX && edge_stride >= num_edges, "shape out of range");
  SPT_CHECK_ARG(num_small >= 0 && num_medium >= 0 && num_small + num_medium <= num_edges,
                "class counts exceed the edges");
  SPT_CHECK_ARG(num_pairs >= 0 && num_pairs <= 0xFFFFFFFFll, "pairs out of range");
  SPT_CHECK_ARG(switches >= 0 && switches < 16, "unknown switch");
  if (num_small + num_medium == 0) return 0;
  SPT_CHECK_ARG(pos && perm && rowptr && edges && anchors && order && count, "null pointer");
  SPT_CHECK_ARG(count_only || edge_attr, "edge_attr is null");
  SPT_CHECK_ARG(count_only || !pair_offset || num_pairs == 0 || (pairs && uid), "pairs / uid is null");
  Params p;
  p.pos = pos; p.num_points = num_points; p.perm = perm; p.rowptr = rowptr;
  p.num_segments = num_segments; p.edges = edges; p.num_edges = num_edges;
  p.edge_stride = edge_stride; p.anchors = anchors;
  p.ratio = ratio; p.margin = margin; p.k_min = k_min; p.switches = switches;
  p.count_only = count_only; p.edge_attr = edge_attr; p.count = count;
  p.pair_offset = count_only ? nullptr : pair_offset;
  p.pairs = pairs; p.uid = uid; p.num_pairs = num_pairs;
  const int64_t cap = 256 * 64;
  if (num_small > 0) {
    p.list = order; p.list_len = num_small;
    superedge_kernel<64, CAP_SMALL><<<(int)(num_small < cap ? num_small : cap), 64, 0, stream>>>(p);
  }
  if (num_medium > 0) {
    p.list = order + num_small; p.list_len = num_medium;
    superedge_kernel<256, CAP_MED><<<(int)(num_medium < cap ? num_medium : cap), 256, 0, stream>>>(p);
  }
  SPT_CHECK_LAUNCH();
  return 0;
}
