// Stride-1 sparse 3D convolution over integer voxel coordinates.
//
// Kernel map: (batch, z, y, x) keys with every axis range padded by r*d (a neighbour position
// outside the cloud's bounds has a key of its own that no voxel holds, so it is absent and never
// aliases), sorted once by the wide-key sort of sorted_runs.hpp; per voxel and per (dz, dy) row one
// binary search and a short walk along x.  Two passes over the same searches - count, then fill -
// around one exclusive scan give the pairs as CSR by output voxel: rowptr [N + 1], and per pair
// the neighbour, the offset index (ascending inside a voxel) and the output voxel.
//
// Forward: output-stationary.  A wave owns 16 consecutive outputs and walks the offsets its rows
// hold in ascending order; for each one the masked [16, C_in] x W[o] product is accumulated in
// registers by v_mfma_f32_16x16x4_f32 (the f32 matrix pipe: exact f32 products, f32 sums).  Each
// output row is written once; no atomics.  A row's sum takes its own offsets in ascending order
// and a zero for the others, so it does not depend on the tile it shares or on the grid.
//
// Backward: dX is the same kernel on the same map (pair (i, o, j) implies (j, K^3 - 1 - o, i))
// with the weight index mirrored and W[o] transposed by the caller.  dW[o] sums x[j]^T gout[i]
// over the pairs of offset o, listed in ascending pair order by one stable sort of the offsets:
// DW_CHUNKS fixed chunks per offset, one wave each, then a post pass adds the chunks in a fixed
// tree.  dbias: DB_PARTS fixed row ranges, then the same post pass.  No float atomics anywhere.
#include "sorted_runs.hpp"

namespace spt {
namespace {

constexpr int THREADS = 256;
constexpr int MAX_C = 64;
constexpr int MAX_K = 15;
constexpr int DW_CHUNKS = 64;
constexpr int DB_PARTS = 1024;

typedef float f32x4 __attribute__((ext_vector_type(4)));

static inline bool count_ok(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31); }

struct MapGeom {
  int64_t origin[4];   // x, y, z, batch: the padded minimum
  int bits[4];
  int K, d;
};

__device__ __forceinline__ uint64_t pack_key(const MapGeom& G, int64_t x, int64_t y, int64_t z,
                                             int64_t b) {
  const int64_t c[4] = {x, y, z, b};
  uint64_t key = 0;
  int shift = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const uint64_t mask = G.bits[a] ? ((~0ull) >> (64 - G.bits[a])) : 0ull;
    key |= ((uint64_t)(c[a] - G.origin[a]) & mask) << shift;
    shift += G.bits[a];
  }
  return key;
}

// ---- bounds --------------------------------------------------------------------------------
__global__ void bounds_init_kernel(long long* __restrict__ rec) {
  if (threadIdx.x < 8)
    rec[threadIdx.x] = (threadIdx.x & 1) ? (long long)INT64_MIN : (long long)INT64_MAX;
}

__global__ __launch_bounds__(THREADS) void bounds_kernel(const int32_t* __restrict__ coords,
                                                         const int64_t* __restrict__ batch,
                                                         int64_t n, long long* __restrict__ rec) {
  long long lo[4], hi[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) { lo[a] = INT64_MAX; hi[a] = INT64_MIN; }
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    long long c[4] = {coords[i * 3], coords[i * 3 + 1], coords[i * 3 + 2], 0};
    if (batch) c[3] = batch[i];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      lo[a] = c[a] < lo[a] ? c[a] : lo[a];
      hi[a] = c[a] > hi[a] ? c[a] : hi[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long l2 = __shfl_xor(lo[a], o, 64), h2 = __shfl_xor(hi[a], o, 64);
      lo[a] = l2 < lo[a] ? l2 : lo[a];
      hi[a] = h2 > hi[a] ? h2 : hi[a];
    }
    if ((threadIdx.x & 63) == 0 && lo[a] <= hi[a]) {
      atomicMin(&rec[2 * a], lo[a]);
      atomicMax(&rec[2 * a + 1], hi[a]);
    }
  }
}

// ---- keys, sorted keys -----------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void keys_kernel(const int32_t* __restrict__ coords,
                                                       const int64_t* __restrict__ batch,
                                                       int64_t n, MapGeom G,
                                                       uint32_t* __restrict__ lo32,
                                                       uint32_t* __restrict__ hi32) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t key = pack_key(G, coords[i * 3], coords[i * 3 + 1], coords[i * 3 + 2],
                                  batch ? batch[i] : 0);
    lo32[i] = (uint32_t)key;
    if (hi32) hi32[i] = (uint32_t)(key >> 32);
  }
}

__global__ void sorted_keys_kernel(SortedKeys keys, int64_t n, uint64_t* __restrict__ skeys,
                                   int32_t* __restrict__ sorder) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
    skeys[t] = sorted_key(keys, t);
    sorder[t] = (int32_t)keys.order[t];
  }
}

// ---- the pairs: count (FILL = false) and fill (FILL = true) ------------------------------------
// One lane per sorted position, so the lanes of a wave search neighbouring keys.  The padded key
// is linear in x inside a row: the neighbours of a (dz, dy) row are the keys of
// [key_lo, key_lo + 2 r d] whose distance from key_lo is a multiple of d.
template <bool FILL>
__global__ __launch_bounds__(THREADS) void map_rows_kernel(
    const int32_t* __restrict__ coords, const int64_t* __restrict__ batch, int64_t n, MapGeom G,
    const uint64_t* __restrict__ skeys, const int32_t* __restrict__ sorder,
    uint32_t* __restrict__ cnt, const int32_t* __restrict__ rowptr, int32_t* __restrict__ nbr,
    int32_t* __restrict__ off, int32_t* __restrict__ row, unsigned long long* __restrict__ rec) {
  const int K = G.K, d = G.d, r = K / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); t0 < n; t0 += stride) {
    const int64_t t = t0 + (threadIdx.x & 63);
    unsigned long long c = 0, dup = 0;
    if (t < n) {
      const int64_t i = sorder[t];
      const int64_t x = coords[i * 3], y = coords[i * 3 + 1], z = coords[i * 3 + 2];
      const int64_t b = batch ? batch[i] : 0;
      int64_t base = 0, end = 0;
      if (FILL) { base = rowptr[i]; end = rowptr[i + 1]; }
      for (int dz = 0; dz < K; ++dz)
        for (int dy = 0; dy < K; ++dy) {
          const uint64_t key_lo = pack_key(G, x - (int64_t)r * d, y + (int64_t)(dy - r) * d,
                                           z + (int64_t)(dz - r) * d, b);
          const uint64_t key_hi = key_lo + (uint64_t)(2 * r * d);
          int64_t lo = 0, hi = n;
          while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (skeys[mid] < key_lo) lo = mid + 1; else hi = mid;
          }
          for (int64_t s = lo; s < n; ++s) {
            const uint64_t k = skeys[s];
            if (k > key_hi) break;
            const uint64_t dxa = k - key_lo;
            if (dxa % (uint64_t)d == 0) {
              if (FILL) {
                const int64_t p = base + (int64_t)c;
                if (p < end) {
                  nbr[p] = sorder[s];
                  off[p] = (dz * K + dy) * K + (int)(dxa / (uint64_t)d);
                  row[p] = (int32_t)i;
                }
              }
              ++c;
            }
          }
        }
      if (!FILL) {
        cnt[i] = (uint32_t)c;
        dup = (t > 0 && skeys[t - 1] == skeys[t]) ? 1ull : 0ull;
      }
    }
    if (!FILL) {
      if (t0 == 0 && (threadIdx.x & 63) == 0) cnt[n] = 0;
      c = wave_reduce_sum(c);
      dup = wave_reduce_sum(dup);
      if ((threadIdx.x & 63) == 0) {
        if (c) atomicAdd(&rec[0], c);
        if (dup) atomicAdd(&rec[1], dup);
      }
    }
  }
}

// ---- forward (and dX) ---------------------------------------------------------------------------
// Lane l of the wave: m = l & 15 is its output row of the tile (operand A) and its column inside
// a 16-column block (operand B, result); g = l >> 4 takes the input channels
// [g * cpl, (g + 1) * cpl), cpl = ceil(C_in / 4): the k index of the 16x16x4 product.  Channels
// and columns beyond C_in / C_out are zeros made in registers, never read.
template <int NT>
__global__ __launch_bounds__(THREADS) void conv_fwd_kernel(
    const float* __restrict__ x, int64_t n, int ci, const float* __restrict__ w, int k3, int co,
    const float* __restrict__ bias, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ nbr, const int32_t* __restrict__ off, int flip,
    float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int m = lane & 15, g = lane >> 4;
  const int64_t row0 = ((int64_t)blockIdx.x * (THREADS / 64) + wv) * 16;
  if (row0 >= n) return;                                   // (wave-uniform)
  const int64_t i = row0 + m;
  int p = 0, e = 0;
  if (i < n) { p = rowptr[i]; e = rowptr[i + 1]; }
  const int cpl = (ci + 3) >> 2;
  const int k0 = g * cpl;
  f32x4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (;;) {
    const int cur = (p < e) ? off[p] : 0x7fffffff;
    int o = cur;
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) {
      const int t = __shfl_xor(o, s, 64);
      o = t < o ? t : o;
    }
    if (o == 0x7fffffff) break;                            // (the four g copies agree: uniform)
    const bool has = cur == o;
    const int64_t j = has ? nbr[p] : 0;
    p += has ? 1 : 0;
    const int ow = flip ? (k3 - 1 - o) : o;
    const float* __restrict__ wo = w + (size_t)ow * ci * co;
    const float* __restrict__ xr = x + (size_t)j * ci;
    for (int kk = 0; kk < cpl; ++kk) {
      const int k = k0 + kk;
      const bool kin = k < ci;
      const float a = (has && kin) ? xr[k] : 0.f;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int col = nt * 16 + m;
        const float b = (kin && col < co) ? wo[(size_t)k * co + col] : 0.f;
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[nt], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int col = nt * 16 + m;
    if (col < co) {
      const float bv = bias ? bias[col] : 0.f;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int64_t orow = row0 + 4 * g + rr;
        if (orow < n) out[(size_t)orow * co + col] = acc[nt][rr] + bv;
      }
    }
  }
}

// ---- dW ---------------------------------------------------------------------------------------
// blockIdx.x = offset, blockIdx.y = chunk of that offset's pairs (4 pairs per product step).
template <int MT, int NT>
__global__ __launch_bounds__(64) void conv_dw_kernel(
    const float* __restrict__ x, const float* __restrict__ gout, int ci, int co,
    const int32_t* __restrict__ nbr, const int32_t* __restrict__ row,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ optr,
    float* __restrict__ partial) {
  const int o = blockIdx.x, c = blockIdx.y;
  const int lane = threadIdx.x, m = lane & 15, g = lane >> 4;
  const int64_t b = optr[o], e = optr[o + 1];
  int64_t len = (e - b + DW_CHUNKS - 1) / DW_CHUNKS;
  len = (len + 3) & ~(int64_t)3;
  const int64_t qb = b + (int64_t)c * len;
  const int64_t qe = (qb + len < e) ? qb + len : e;
  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int64_t q = qb; q < qe; q += 4) {
    const int64_t qq = q + g;
    const bool ok = qq < qe;
    const int p = ok ? perm[qq] : 0;
    const int64_t j = ok ? nbr[p] : 0;
    const int64_t i = ok ? row[p] : 0;
    float a[MT], bb[NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int k = mt * 16 + m;
      a[mt] = (ok && k < ci) ? x[(size_t)j * ci + k] : 0.f;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = nt * 16 + m;
      bb[nt] = (ok && col < co) ? gout[(size_t)i * co + col] : 0.f;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], bb[nt], acc[mt][nt], 0, 0, 0);
  }
  float* __restrict__ po = partial + ((size_t)o * DW_CHUNKS + c) * ci * co;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = nt * 16 + m;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int k = mt * 16 + 4 * g + rr;
        if (k < ci && col < co) po[(size_t)k * co + col] = acc[mt][nt][rr];
      }
    }
}

// partial [groups][parts][len] -> out [groups][len].  The parts are added in a FIXED tree: eight
// consecutive parts pairwise, eight of those sums pairwise, and the sums of 64 parts one after
// the other from part 0 - at most 6 + parts / 64 roundings on a term instead of `parts`.
__device__ __forceinline__ float tree8(const float* v) {
  return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

__global__ void sum_parts_kernel(const float* __restrict__ partial, int64_t groups, int parts,
                                 int64_t len, float* __restrict__ out) {
  const int64_t total = groups * len;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t gidx = t / len, el = t - gidx * len;
    const float* __restrict__ src = partial + (size_t)gidx * parts * len + el;
    float s = 0.f;
    for (int c0 = 0; c0 < parts; c0 += 64) {
      float s2[8];
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int c = c0 + b * 8 + u;
          v[u] = c < parts ? src[(size_t)c * len] : 0.f;
        }
        s2[b] = tree8(v);
      }
      s += tree8(s2);
    }
    out[t] = s;
  }
}

// ---- dbias --------------------------------------------------------------------------------------
// part = blockIdx.x: rows [part * len, ...), one lane per column: eight consecutive rows pairwise,
// those sums one after the other from the first
__global__ __launch_bounds__(64) void conv_dbias_kernel(const float* __restrict__ gout, int64_t n,
                                                        int co, float* __restrict__ partial) {
  const int64_t len = (n + DB_PARTS - 1) / DB_PARTS;
  const int64_t b = (int64_t)blockIdx.x * len;
  const int64_t e = (b + len < n) ? b + len : n;
  const int col = threadIdx.x;
  if (col >= co) return;
  float s = 0.f;
  for (int64_t i0 = b; i0 < e; i0 += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = (i0 + u < e) ? gout[(size_t)(i0 + u) * co + col] : 0.f;
    s += tree8(v);
  }
  partial[(size_t)blockIdx.x * co + col] = s;
}

// the sort (csrc/sorted_runs.hpp), the permutation it borrows for a key of two words, and the
// partials of the scan over rowptr
struct CountPlan {
  SortPlan sort;
  size_t off_perm, off_part, total;
  int64_t part_cap;
};

CountPlan count_plan(int64_t n, int key_bits) {
  CountPlan p;
  p.sort = sort_plan(n, key_bits);
  size_t off = p.sort.total;
  p.off_perm = off; off += key_bits > 32 ? align_up((size_t)n * 4, 256) : 0;
  p.off_part = off; off += scan_part_bytes(n + 1);
  p.part_cap = (int64_t)(scan_part_bytes(n + 1) / 4);
  p.total = off;
  return p;
}

int read_geom(const int64_t* origin, const int* bits, int kernel_size, int dilation,
              bool has_batch, MapGeom* G, int* key_bits) {
  int kb = 0;
  for (int a = 0; a < 4; ++a) {
    if (bits[a] < 0 || bits[a] > 33) return -1;
    G->origin[a] = origin[a];
    G->bits[a] = bits[a];
    kb += bits[a];
  }
  if (!has_batch && bits[3] != 0) return -1;
  if (kb < 1 || kb > 63) return -1;
  G->K = kernel_size;
  G->d = dilation;
  *key_bits = kb;
  return 0;
}

bool geom_args_ok(int kernel_size, int dilation) {
  return kernel_size >= 1 && kernel_size <= MAX_K && (kernel_size & 1) && dilation >= 1 &&
         dilation <= (1 << 20);
}

}  // namespace
}  // namespace spt

using namespace spt;

extern "C" int spt_sparse_bounds_i32(const int32_t* coords, const int64_t* batch, int64_t n,
                                     int64_t* record, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "n out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(coords && record, "null pointer");
  bounds_init_kernel<<<1, 64, 0, stream>>>((long long*)record);
  bounds_kernel<<<stream_grid(n, THREADS * 4), THREADS, 0, stream>>>(coords, batch, n,
                                                                      (long long*)record);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_sparse_map_count_workspace_bytes(int64_t n, int key_bits) {
  if (!count_ok(n) || n < 1 || key_bits < 1 || key_bits > 63) return 0;
  return count_plan(n, key_bits).total;
}

extern "C" int spt_sparse_map_count(const int32_t* coords, const int64_t* batch, int64_t n,
                                    const int64_t* origin, const int* bits, int kernel_size,
                                    int dilation, uint64_t* skeys, int32_t* sorder,
                                    int32_t* rowptr, int64_t* record, void* ws, size_t ws_bytes,
                                    spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "n out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(coords && origin && bits && skeys && sorder && rowptr && record, "null pointer");
  SPT_CHECK_ARG(geom_args_ok(kernel_size, dilation),
                "kernel_size must be odd in 1 .. 15 and dilation in 1 .. 2^20");
  MapGeom G;
  int key_bits = 0;
  SPT_CHECK_ARG(read_geom(origin, bits, kernel_size, dilation, batch != nullptr, &G, &key_bits) == 0,
                "the key fields must add up to 1 .. 63 bits (batch bits only with a batch)");
  const CountPlan p = count_plan(n, key_bits);
  SPT_CHECK_ARG(ws && ws_bytes >= p.total, "workspace too small");
  char* base = (char*)ws;
  const WideKeys keys = sort_carve(base, p.sort);
  uint32_t* perm = (uint32_t*)(base + p.off_perm);
  uint32_t* part = (uint32_t*)(base + p.off_part);

  SPT_CHECK_ARG(hipMemsetAsync(record, 0, 2 * sizeof(int64_t), stream) == hipSuccess,
                "could not queue the record reset");
  const int g = stream_grid(n, THREADS);
  keys_kernel<<<g, THREADS, 0, stream>>>(coords, batch, n, G, keys.minor, keys.major);
  SortedKeys sorted;
  SPT_CHECK_ARG(sort_wide(base, p.sort, n, perm, stream, &sorted) == 0, "sort scratch too small");
  sorted_keys_kernel<<<g, THREADS, 0, stream>>>(sorted, n, skeys, sorder);
  map_rows_kernel<false><<<g, THREADS, 0, stream>>>(coords, batch, n, G, skeys, sorder,
                                                    (uint32_t*)rowptr, nullptr, nullptr, nullptr,
                                                    nullptr, (unsigned long long*)record);
  SPT_CHECK_ARG(device_exclusive_scan((uint32_t*)rowptr, n + 1, part, p.part_cap, stream) == 0,
                "scan partials too small");
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_sparse_map_fill(const int32_t* coords, const int64_t* batch, int64_t n,
                                   const int64_t* origin, const int* bits, int kernel_size,
                                   int dilation, const uint64_t* skeys, const int32_t* sorder,
                                   const int32_t* rowptr, int64_t num_pairs, int32_t* nbr,
                                   int32_t* off, int32_t* row, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "n out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(count_ok(num_pairs) && num_pairs >= 1, "num_pairs out of range (1 <= P < 2^31)");
  SPT_CHECK_ARG(coords && origin && bits && skeys && sorder && rowptr && nbr && off && row,
                "null pointer");
  SPT_CHECK_ARG(geom_args_ok(kernel_size, dilation),
                "kernel_size must be odd in 1 .. 15 and dilation in 1 .. 2^20");
  MapGeom G;
  int key_bits = 0;
  SPT_CHECK_ARG(read_geom(origin, bits, kernel_size, dilation, batch != nullptr, &G, &key_bits) == 0,
                "the key fields must add up to 1 .. 63 bits (batch bits only with a batch)");
  map_rows_kernel<true><<<stream_grid(n, THREADS), THREADS, 0, stream>>>(
      coords, batch, n, G, skeys, sorder, nullptr, rowptr, nbr, off, row, nullptr);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_sparse_map_by_offset_workspace_bytes(int64_t num_pairs) {
  if (!count_ok(num_pairs) || num_pairs < 1) return 0;
  return RadixScratch::bytes(num_pairs);
}

extern "C" int spt_sparse_map_by_offset(const int32_t* off, int64_t num_pairs, int k3,
                                        int32_t* perm, int32_t* optr, void* ws, size_t ws_bytes,
                                        spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(num_pairs) && num_pairs >= 1, "num_pairs out of range (1 <= P < 2^31)");
  SPT_CHECK_ARG(k3 >= 1 && k3 <= MAX_K * MAX_K * MAX_K, "k3 out of range");
  SPT_CHECK_ARG(off && perm && optr, "null pointer");
  SPT_CHECK_ARG(ws && ws_bytes >= RadixScratch::bytes(num_pairs), "workspace too small");
  RadixScratch s;
  s.carve((char*)ws, num_pairs);
  const uint32_t *ks = nullptr, *vs = nullptr;
  SPT_CHECK_ARG(radix_sort_pairs<2>(nullptr, (const uint32_t*)off, nullptr, num_pairs,
                                    bits_for(k3), s, (uint32_t*)perm, &ks, &vs, stream) == 0,
                "sort scratch too small");
  rowptr_from_sorted_kernel<<<stream_grid(num_pairs + 1, THREADS), THREADS, 0, stream>>>(
      ks, num_pairs, k3, optr);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_sparse_conv_supported(int c_in, int c_out) {
  return c_in >= 1 && c_in <= MAX_C && c_out >= 16 && c_out <= MAX_C && c_out % 16 == 0;
}

extern "C" int spt_sparse_conv_fwd_f32(const float* x, int64_t n, int c_in, const float* w, int k3,
                                       int c_out, const float* bias, const int32_t* rowptr,
                                       const int32_t* nbr, const int32_t* off, int flip,
                                       float* out, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "n out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(c_in >= 1 && c_in <= MAX_C && c_out >= 1 && c_out <= MAX_C,
                "channels out of range (1 .. 64)");
  SPT_CHECK_ARG(k3 >= 1 && k3 <= MAX_K * MAX_K * MAX_K, "k3 out of range");
  SPT_CHECK_ARG(x && w && rowptr && nbr && off && out, "null pointer");
  SPT_CHECK_ARG(out != x, "out must not alias x");
  const int64_t tiles = ceil_div(n, 16);
  const unsigned grid = (unsigned)ceil_div(tiles, THREADS / 64);
  const int nt = (c_out + 15) / 16;
#define SPT_FWD(NT)                                                                          \
  conv_fwd_kernel<NT><<<grid, THREADS, 0, stream>>>(x, n, c_in, w, k3, c_out, bias, rowptr, \
                                                    nbr, off, flip ? 1 : 0, out)
  switch (nt) {
    case 1: SPT_FWD(1); break;
    case 2: SPT_FWD(2); break;
    case 3: SPT_FWD(3); break;
    default: SPT_FWD(4); break;
  }
#undef SPT_FWD
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_sparse_conv_dw_workspace_bytes(int k3, int c_in, int c_out) {
  if (k3 < 1 || k3 > MAX_K * MAX_K * MAX_K || c_in < 1 || c_in > MAX_C || c_out < 1 ||
      c_out > MAX_C)
    return 0;
  return align_up((size_t)k3 * DW_CHUNKS * c_in * c_out * 4, 256);
}

extern "C" int spt_sparse_conv_dw_f32(const float* x, const float* gout, int64_t n, int c_in,
                                      int c_out, int k3, const int32_t* nbr, const int32_t* row,
                                      const int32_t* perm, const int32_t* optr, int64_t num_pairs,
                                      float* dw, void* ws, size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "n out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(count_ok(num_pairs) && num_pairs >= 1, "num_pairs out of range (1 <= P < 2^31)");
  SPT_CHECK_ARG(c_in >= 1 && c_in <= MAX_C && c_out >= 1 && c_out <= MAX_C,
                "channels out of range (1 .. 64)");
  SPT_CHECK_ARG(k3 >= 1 && k3 <= MAX_K * MAX_K * MAX_K, "k3 out of range");
  SPT_CHECK_ARG(x && gout && nbr && row && perm && optr && dw, "null pointer");
  const size_t need = spt_sparse_conv_dw_workspace_bytes(k3, c_in, c_out);
  SPT_CHECK_ARG(ws && ws_bytes >= need, "workspace too small");
  float* partial = (float*)ws;
  const dim3 grid(k3, DW_CHUNKS);
  const int mt = (c_in + 15) / 16, nt = (c_out + 15) / 16;
#define SPT_DW(MT, NT)                                                                         \
  conv_dw_kernel<MT, NT><<<grid, 64, 0, stream>>>(x, gout, c_in, c_out, nbr, row, perm, optr, \
                                                  partial)
#define SPT_DW_N(MT)              \
  switch (nt) {                   \
    case 1: SPT_DW(MT, 1); break; \
    case 2: SPT_DW(MT, 2); break; \
    case 3: SPT_DW(MT, 3); break; \
    default: SPT_DW(MT, 4); break; \
  }
  switch (mt) {
    case 1: SPT_DW_N(1); break;
    case 2: SPT_DW_N(2); break;
    case 3: SPT_DW_N(3); break;
    default: SPT_DW_N(4); break;
  }
#undef SPT_DW_N
#undef SPT_DW
  const int64_t len = (int64_t)c_in * c_out;
  sum_parts_kernel<<<stream_grid((int64_t)k3 * len, THREADS), THREADS, 0, stream>>>(
      partial, k3, DW_CHUNKS, len, dw);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_sparse_conv_dbias_workspace_bytes(int c_out) {
  if (c_out < 1 || c_out > MAX_C) return 0;
  return align_up((size_t)DB_PARTS * c_out * 4, 256);
}

extern "C" int spt_sparse_conv_dbias_f32(const float* gout, int64_t n, int c_out, float* dbias,
                                         void* ws, size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(count_ok(n) && n >= 1, "n out of range (1 <= n < 2^31)");
  SPT_CHECK_ARG(c_out >= 1 && c_out <= MAX_C, "c_out out of range (1 .. 64)");
  SPT_CHECK_ARG(gout && dbias, "null pointer");
  SPT_CHECK_ARG(ws && ws_bytes >= spt_sparse_conv_dbias_workspace_bytes(c_out),
                "workspace too small");
  float* partial = (float*)ws;
  conv_dbias_kernel<<<DB_PARTS, 64, 0, stream>>>(gout, n, c_out, partial);
  sum_parts_kernel<<<1, 64, 0, stream>>>(partial, 1, DB_PARTS, c_out, dbias);
  SPT_CHECK_LAUNCH();
  return 0;
}
