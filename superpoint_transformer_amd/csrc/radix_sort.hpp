// Stable LSD radix sort of (u32 key, u32 value) pairs + device-wide u32 scan,
// shared by the CSR builder (csr_build.hip) and the segment sampler
// (sampling.hip).  gfx950 only: wave64 ballots rank equal digits inside a wave,
// 4-wave workgroups, LDS digit counters, <= 8 bits per pass.
//
// First-pass source (template MODE of the hist / scatter kernels):
//   0  u32 keys + u32 values            (every later pass)
//   1  int64 index array, values = iota (CSR build)
//   2  u32 keys, values = iota
#pragma once
#include "common.hpp"

namespace spt {


constexpr int SORT_THREADS = 256;
constexpr int SORT_WAVES = SORT_THREADS / 64;
constexpr int SORT_ITEMS = 16;                        // keys per lane
constexpr int SORT_TILE = SORT_THREADS * SORT_ITEMS;  // 4096 keys per workgroup
constexpr int WAVE_CHUNK = SORT_TILE / SORT_WAVES;    // 1024 consecutive keys per wave
constexpr int MAX_BINS = 256;

template <int MODE>
__device__ __forceinline__ uint32_t load_key(const int64_t* __restrict__ idx,
                                             const uint32_t* __restrict__ keys,
                                             int64_t i) {
  if constexpr (MODE == 1)
    return (uint32_t)idx[i];
  else
    return keys[i];
}

// ---- per-workgroup digit histogram -----------------------------------------
template <int MODE>
__global__ __launch_bounds__(SORT_THREADS) void radix_hist_kernel(
    const int64_t* __restrict__ idx, const uint32_t* __restrict__ keys_in,
    int64_t n, int shift, int bits, uint32_t* __restrict__ blockhist,
    int nblocks) {
  __shared__ uint32_t h[MAX_BINS];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SORT_TILE;
  const uint32_t mask = (1u << bits) - 1u;
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; ++k) {
    int64_t i = base + (int64_t)k * SORT_THREADS + threadIdx.x;
    if (i < n) {
      uint32_t d = (load_key<MODE>(idx, keys_in, i) >> shift) & mask;
      atomicAdd(&h[d], 1u);
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < (1 << bits))
    blockhist[(size_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

// ---- stable scatter ----------------------------------------------------------
// Order inside a tile is (wave, round, lane) == ascending input position, so
// equal digits keep their relative order: the sort is stable.
template <int MODE>
__global__ __launch_bounds__(SORT_THREADS) void radix_scatter_kernel(
    const int64_t* __restrict__ idx, const uint32_t* __restrict__ keys_in,
    const uint32_t* __restrict__ vals_in, int64_t n, int shift, int bits,
    const uint32_t* __restrict__ blockoff, int nblocks,
    uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
  __shared__ uint32_t cnt[SORT_WAVES][MAX_BINS];
  const int w = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  for (int j = threadIdx.x; j < SORT_WAVES * MAX_BINS; j += SORT_THREADS)
    (&cnt[0][0])[j] = 0;
  __syncthreads();

  const int64_t wbase = (int64_t)blockIdx.x * SORT_TILE + (int64_t)w * WAVE_CHUNK;
  const uint32_t mask = (1u << bits) - 1u;
  const uint64_t lt = lanemask_lt();

  uint32_t key[SORT_ITEMS];
  uint32_t rank[SORT_ITEMS];
#pragma unroll
  for (int r = 0; r < SORT_ITEMS; ++r) {
    int64_t i = wbase + r * 64 + lane;
    key[r] = (i < n) ? load_key<MODE>(idx, keys_in, i) : 0xffffffffu;
  }
#pragma unroll
  for (int r = 0; r < SORT_ITEMS; ++r) {
    const int64_t i = wbase + r * 64 + lane;
    const bool valid = i < n;
    const uint32_t d = (key[r] >> shift) & mask;
    uint64_t peers = __ballot(valid);
    for (int b = 0; b < bits; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(valid && bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t pre = cnt[w][d];
    const uint32_t rk = __popcll(peers & lt);
    const uint32_t tot = __popcll(peers);
    rank[r] = pre + rk;
    __builtin_amdgcn_wave_barrier();
    if (valid && rk == tot - 1) cnt[w][d] = pre + tot;  // highest peer lane
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  if ((int)threadIdx.x < (1 << bits)) {
    const int d = threadIdx.x;
    uint32_t base = blockoff[(size_t)d * nblocks + blockIdx.x];
#pragma unroll
    for (int w2 = 0; w2 < SORT_WAVES; ++w2) {
      uint32_t t = cnt[w2][d];
      cnt[w2][d] = base;
      base += t;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_ITEMS; ++r) {
    const int64_t i = wbase + r * 64 + lane;
    if (i < n) {
      const uint32_t d = (key[r] >> shift) & mask;
      const uint32_t dst = cnt[w][d] + rank[r];
      keys_out[dst] = key[r];
      if constexpr (MODE != 0)
        vals_out[dst] = (uint32_t)i;
      else
        vals_out[dst] = vals_in[i];
    }
  }
}

// ---- device-wide exclusive scan (3 launches) -------------------------------
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 16;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

// Partials of a scan over m values: one u32 per SCAN_TILE chunk.  The ONLY formula for that
// region - every plan that feeds device_exclusive_scan sizes its partials with it, for the
// longest array it scans.
static inline int64_t scan_part_entries(int64_t m) { return ceil_div(m > 0 ? m : 1, SCAN_TILE); }
static inline size_t scan_part_bytes(int64_t m) {
  return align_up((size_t)scan_part_entries(m) * 4, 256);
}

// The common scratch of "flag / count array of m u32 values, scanned in place": the array, then
// its partials.  `part_cap` is what the layout reserved, in entries - the capacity a caller
// hands to device_exclusive_scan.
struct ScanPlan {
  size_t off_part, total;
  int64_t part_cap;
};
static inline ScanPlan scan_plan(int64_t m) {
  ScanPlan p;
  p.off_part = align_up((size_t)(m > 0 ? m : 1) * 4, 256);
  p.total = p.off_part + scan_part_bytes(m);
  p.part_cap = (int64_t)((p.total - p.off_part) / 4);
  return p;
}

__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v,
                                                         uint32_t* total) {
  __shared__ uint32_t wsum[SCAN_THREADS / 64];
  const int w = threadIdx.x >> 6;
  const uint32_t inc = wave_inclusive_scan(v);
  __syncthreads();  // protects wsum reuse across calls
  if ((threadIdx.x & 63) == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t off = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < SCAN_THREADS / 64; ++k) {
    uint32_t s = wsum[k];
    if (k < w) off += s;
    tot += s;
  }
  if (total) *total = tot;
  return off + inc - v;
}

static __global__ __launch_bounds__(SCAN_THREADS) void scan_reduce_kernel(
    const uint32_t* __restrict__ in, int64_t m, uint32_t* __restrict__ partial) {
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k)
    if (base + k < m) s += in[base + k];
  uint32_t tot;
  block_exclusive_scan(s, &tot);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// single workgroup: exclusive scan of the chunk totals, carry across rounds
static __global__ __launch_bounds__(SCAN_THREADS) void scan_partials_kernel(
    uint32_t* __restrict__ partial, int nchunks) {
  uint32_t carry = 0;
  for (int base = 0; base < nchunks; base += SCAN_THREADS) {
    const int i = base + threadIdx.x;
    const uint32_t v = (i < nchunks) ? partial[i] : 0u;
    uint32_t tot;
    const uint32_t ex = block_exclusive_scan(v, &tot);
    if (i < nchunks) partial[i] = carry + ex;
    carry += tot;
  }
}

static __global__ __launch_bounds__(SCAN_THREADS) void scan_apply_kernel(
    uint32_t* __restrict__ data, int64_t m, const uint32_t* __restrict__ partial) {
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS];
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    v[k] = (base + k < m) ? data[base + k] : 0u;
    s += v[k];
  }
  uint32_t run = block_exclusive_scan(s, nullptr) + partial[blockIdx.x];
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    if (base + k < m) data[base + k] = run;
    run += v[k];
  }
}

// ---- boundaries of the sorted key array -> rowptr ----------------------------
// rowptr[s] = first position of a key >= s.  Element i owns the entries (skeys[i-1], skeys[i]]:
// one for a dense id space, but a sparse one (the cells of a kNN grid over surfaces: most of the
// volume is empty) has runs of thousands of empty ids between two occupied ones - a lane filling
// its run alone kept the whole launch waiting (5.4 ms for 29 M cells / 12 M points).  Runs longer
// than 4 entries are filled by the whole wave, 64 consecutive entries per store.
static __global__ void rowptr_from_sorted_kernel(const uint32_t* __restrict__ skeys,
                                          int64_t n, int64_t num_seg,
                                          int32_t* __restrict__ rowptr) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base <= n;
       base += stride) {                                  // (wave-uniform trip count)
    const int64_t i = base + lane;
    int64_t lo = 0, hi = -1;  // rowptr[lo+1 .. hi] = i
    if (i <= n) {
      if (i == n) {
        lo = (n > 0) ? (int64_t)skeys[n - 1] : -1;
        hi = num_seg;
      } else {
        hi = (int64_t)skeys[i];
        lo = (i > 0) ? (int64_t)skeys[i - 1] : -1;
      }
      if (lo > num_seg - 1) lo = num_seg - 1;  // out-of-range keys: stay in bounds
      if (hi > num_seg) hi = num_seg;
      if (i < n && hi > num_seg - 1) hi = num_seg - 1;
    }
    const bool longrun = hi - lo > 4;
    if (!longrun)
      for (int64_t s = lo + 1; s <= hi; ++s) rowptr[s] = (int32_t)i;
    uint64_t todo = __ballot(longrun);
    while (todo) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const int64_t l2 = __shfl(lo, src, 64), h2 = __shfl(hi, src, 64);
      const int32_t v = (int32_t)(base + src);
      for (int64_t s = l2 + 1 + lane; s <= h2; s += 64) rowptr[s] = v;
    }
  }
}

static __global__ void iota_kernel(int32_t* __restrict__ perm, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    perm[i] = (int32_t)i;
}

static __global__ void rowptr_single_kernel(int32_t* rowptr, int64_t n) {
  rowptr[0] = 0;
  rowptr[1] = (int32_t)n;
}


static inline int bits_for(int64_t num_seg) {
  int b = 1;
  while (((int64_t)1 << b) < num_seg) ++b;
  return b;
}

// Scratch of one sort: two key buffers, two value buffers, per-workgroup digit
// histograms and scan partials.  `bytes(n)` is what `carve` consumes.  `part` holds
// `part_cap` entries: enough for the digit histograms of a sort of n keys and for nothing
// longer - a caller that scans another array brings partials of its own.
struct RadixScratch {
  uint32_t *k0, *k1, *v0, *v1, *hist, *part;
  int64_t part_cap;
  static size_t bytes(int64_t n) {
    const int64_t m = n > 0 ? n : 1;
    const int nblocks = (int)ceil_div(m, SORT_TILE);
    const int64_t hist_len = (int64_t)MAX_BINS * nblocks;
    return 4 * align_up((size_t)m * 4, 256) + align_up((size_t)hist_len * 4, 256) +
           scan_part_bytes(hist_len);
  }
  char* carve(char* base, int64_t n) {
    const int64_t m = n > 0 ? n : 1;
    const size_t nb = align_up((size_t)m * 4, 256);
    const int nblocks = (int)ceil_div(m, SORT_TILE);
    const int64_t hist_len = (int64_t)MAX_BINS * nblocks;
    k0 = (uint32_t*)base; base += nb;
    k1 = (uint32_t*)base; base += nb;
    v0 = (uint32_t*)base; base += nb;
    v1 = (uint32_t*)base; base += nb;
    hist = (uint32_t*)base; base += align_up((size_t)hist_len * 4, 256);
    part = (uint32_t*)base; base += scan_part_bytes(hist_len);
    part_cap = (int64_t)(scan_part_bytes(hist_len) / 4);
    return base;
  }
};

// In-place exclusive scan of m u32 values (3 launches).  `part` has room for `part_cap`
// entries; the scan writes scan_part_entries(m) of them.  Returns 0, or -1 WITHOUT launching
// anything when the partials would not fit (callers: SPT_CHECK_ARG on the result).
static inline int device_exclusive_scan(uint32_t* data, int64_t m, uint32_t* part,
                                        int64_t part_cap, hipStream_t stream) {
  if (scan_part_entries(m) > part_cap) return -1;
  const int nch = (int)scan_part_entries(m);
  scan_reduce_kernel<<<nch, SCAN_THREADS, 0, stream>>>(data, m, part);
  scan_partials_kernel<<<1, SCAN_THREADS, 0, stream>>>(part, nch);
  scan_apply_kernel<<<nch, SCAN_THREADS, 0, stream>>>(data, m, part);
  return 0;
}

// Sort n pairs by the low `nbits` bits of the key.  MODE selects the first-pass
// source (see top).  The last pass writes its values to `final_vals` when given
// (else into the scratch); returns the sorted keys / values through the out
// pointers.  nbits >= 1, n >= 1.  Returns 0, or -1 when the scratch's partials are too small
// for a pass's histogram (nothing of that pass is launched).
template <int MODE>
static inline int radix_sort_pairs(const int64_t* idx64, const uint32_t* keys32,
                                    const uint32_t* vals32, int64_t n, int nbits,
                                    RadixScratch& s, uint32_t* final_vals,
                                    const uint32_t** keys_sorted,
                                    const uint32_t** vals_sorted, hipStream_t stream) {
  const int nblocks = (int)ceil_div(n, SORT_TILE);
  const int passes = (nbits + 7) / 8;
  const int per = (nbits + passes - 1) / passes;   // balanced digits, e.g. 19 -> 7+6+6
  if (scan_part_entries((int64_t)(1 << per) * nblocks) > s.part_cap) return -1;  // widest pass
  uint32_t* kbuf[2] = {s.k0, s.k1};
  uint32_t* vbuf[2] = {s.v0, s.v1};
  const uint32_t* kin = keys32;
  const uint32_t* vin = vals32;
  int shift = 0;
  for (int pass = 0; pass < passes; ++pass) {
    const int bits = (nbits - shift < per) ? (nbits - shift) : per;
    uint32_t* kout = kbuf[pass & 1];
    uint32_t* vout = vbuf[pass & 1];
    if (pass == passes - 1 && final_vals) vout = final_vals;
    const int64_t hl = (int64_t)(1 << bits) * nblocks;
    if (pass == 0) {
      radix_hist_kernel<MODE><<<nblocks, SORT_THREADS, 0, stream>>>(
          idx64, kin, n, shift, bits, s.hist, nblocks);
      if (device_exclusive_scan(s.hist, hl, s.part, s.part_cap, stream)) return -1;
      radix_scatter_kernel<MODE><<<nblocks, SORT_THREADS, 0, stream>>>(
          idx64, kin, vin, n, shift, bits, s.hist, nblocks, kout, vout);
    } else {
      radix_hist_kernel<0><<<nblocks, SORT_THREADS, 0, stream>>>(
          nullptr, kin, n, shift, bits, s.hist, nblocks);
      if (device_exclusive_scan(s.hist, hl, s.part, s.part_cap, stream)) return -1;
      radix_scatter_kernel<0><<<nblocks, SORT_THREADS, 0, stream>>>(
          nullptr, kin, vin, n, shift, bits, s.hist, nblocks, kout, vout);
    }
    kin = kout;
    vin = vout;
    shift += bits;
  }
  *keys_sorted = kin;
  *vals_sorted = vin;
  return 0;
}

// ---- the edge sort: (key, value, target) triples, tables out of the last pass ---------------------
// The sort of an attention graph's edges by source (csr_build.hip: spt_edge_csr_build).  Same
// tile, same (wave, round, lane) order, same ballot ranking and the same <= 8-bit balanced digits
// as above, so it is stable and gives the one result the pair sort gives.  What differs:
//   * the per-workgroup histograms [digit][workgroup] are scanned ROW BY ROW by one launch
//     (edge_rowscan_kernel: a workgroup per digit, which also leaves the digit's total); the
//     scatter kernel scans the <= 256 digit totals itself to find where a digit starts.  One scan
//     launch per pass instead of three, no partials region;
//   * the first histogram kernel reads the int64 sources and, when the caller declared a mirror
//     count, checks that structure on the way (one verdict word per workgroup, OR-ed by the row
//     scan: no atomics on the flag, nothing to clear);
//   * the scatter kernel puts its tile in digit order in LDS before it writes, so the elements
//     of one digit leave as ONE run of consecutive addresses from consecutive lanes (a store
//     per input element touched up to 64 lines per instruction: 76 - 136 us per pass over 7 M
//     edges for pairs, against 62 - 70 us staged for triples);
//   * the target of every edge travels with it (read once, in order, by the first pass), so the
//     last pass writes tgt_sorted without a random 8-byte gather; it also writes inv[value].
// Wider digits (up to 11 bits: two passes for 2^19 nodes) were built and measured: the last pass
// then took 235 us against 83 us (runs of 4 elements per digit and tile), 583 against 527 us
// per level-1 build - three passes stay.

// FIRST: keys = (u32) ei[0 .. n), checks [i<j | j>i | loops] with `pairs` = M (< 0: no check).
template <bool FIRST>
__global__ __launch_bounds__(SORT_THREADS) void edge_hist_kernel(
    const int64_t* __restrict__ ei, const uint32_t* __restrict__ keys_in, int64_t n, int shift,
    int bits, uint32_t* __restrict__ blockhist, int nblocks, int64_t pairs,
    uint32_t* __restrict__ blockbad) {
  __shared__ uint32_t h[MAX_BINS];
  __shared__ uint32_t sbad;
  h[threadIdx.x] = 0;
  if (threadIdx.x == 0) sbad = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SORT_TILE;
  const uint32_t mask = (1u << bits) - 1u;
  uint32_t bad = 0;
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; ++k) {
    const int64_t i = base + (int64_t)k * SORT_THREADS + threadIdx.x;
    if (i < n) {
      uint32_t key;
      if constexpr (FIRST) {
        const int64_t s = ei[i];
        key = (uint32_t)s;
        if (pairs >= 0) {
          const int64_t t = ei[n + i];
          if (i < pairs) {
            if (ei[i + pairs] != t || ei[n + i + pairs] != s) bad |= 1u;
          } else if (i >= 2 * pairs) {
            if (s != t) bad |= 2u;
          }
        }
      } else {
        key = keys_in[i];
      }
      atomicAdd(&h[(key >> shift) & mask], 1u);
    }
  }
  if constexpr (FIRST)
    if (bad) atomicOr(&sbad, bad);
  __syncthreads();
  if ((int)threadIdx.x < (1 << bits))
    blockhist[(size_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
  if constexpr (FIRST)
    if (threadIdx.x == 0) blockbad[blockIdx.x] = sbad;
}

// Workgroup d: exclusive scan of row d of blockhist in place, the row's total to digit_total[d].
// Workgroup 0 also ORs the per-workgroup verdicts into *flag (flag == nullptr: no verdicts).
static __global__ __launch_bounds__(SCAN_THREADS) void edge_rowscan_kernel(
    uint32_t* __restrict__ blockhist, int nblocks, uint32_t* __restrict__ digit_total,
    const uint32_t* __restrict__ blockbad, int32_t* __restrict__ flag) {
  uint32_t* row = blockhist + (size_t)blockIdx.x * nblocks;
  uint32_t carry = 0;
  for (int base = 0; base < nblocks; base += SCAN_THREADS) {
    const int i = base + threadIdx.x;
    const uint32_t v = (i < nblocks) ? row[i] : 0u;
    uint32_t tot;
    const uint32_t ex = block_exclusive_scan(v, &tot);
    if (i < nblocks) row[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) digit_total[blockIdx.x] = carry;
  if (blockIdx.x == 0 && flag) {
    __shared__ uint32_t sbad;
    if (threadIdx.x == 0) sbad = 0;
    __syncthreads();
    uint32_t bad = 0;
    for (int i = threadIdx.x; i < nblocks; i += SCAN_THREADS) bad |= blockbad[i];
    if (bad) atomicOr(&sbad, bad);
    __syncthreads();
    if (threadIdx.x == 0) *flag = (int32_t)sbad;
  }
}

// MODE 1: key = (u32) ei[i], value = i, target = (i32) ei[n + i];  MODE 0: the three input arrays.
// LAST: also inv[value] = destination (inv may be null).
template <int MODE, bool LAST>
__global__ __launch_bounds__(SORT_THREADS) void edge_scatter_kernel(
    const int64_t* __restrict__ ei, const uint32_t* __restrict__ keys_in,
    const uint32_t* __restrict__ vals_in, const int32_t* __restrict__ tgts_in, int64_t n, int shift,
    int bits, const uint32_t* __restrict__ blockoff, const uint32_t* __restrict__ digit_total,
    int nblocks, uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out,
    int32_t* __restrict__ tgts_out, int32_t* __restrict__ inv) {
  // the counters [wave][MAX_BINS]; once every element knows its slot, the staged tile
  // (keys | values | targets) takes over their words
  __shared__ uint32_t buf[3 * SORT_TILE];
  __shared__ uint32_t dbase[MAX_BINS];  // where a digit starts; later: destination - slot of the digit
  __shared__ uint32_t texcl[MAX_BINS];  // first slot of a digit in the staged tile
  static_assert(SORT_WAVES * MAX_BINS <= 3 * SORT_TILE && MAX_BINS == SORT_THREADS, "LDS plan");
  uint32_t(*cnt)[MAX_BINS] = reinterpret_cast<uint32_t(*)[MAX_BINS]>(buf);
  const int w = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int bins = 1 << bits;
  const bool own = (int)threadIdx.x < bins;     // this thread owns digit threadIdx.x
  for (int j = threadIdx.x; j < SORT_WAVES * MAX_BINS; j += SORT_THREADS) buf[j] = 0;

  const int64_t tbase = (int64_t)blockIdx.x * SORT_TILE;
  const int64_t wbase = tbase + (int64_t)w * WAVE_CHUNK;
  const uint32_t mask = (uint32_t)bins - 1u;
  const uint64_t lt = lanemask_lt();

  uint32_t key[SORT_ITEMS];
  uint32_t val[SORT_ITEMS];
  int32_t tgt[SORT_ITEMS];
  uint32_t rank[SORT_ITEMS];
#pragma unroll
  for (int r = 0; r < SORT_ITEMS; ++r) {
    const int64_t i = wbase + r * 64 + lane;
    const bool valid = i < n;
    if constexpr (MODE == 1) {
      key[r] = valid ? (uint32_t)ei[i] : 0xffffffffu;
      val[r] = (uint32_t)i;
      tgt[r] = valid ? (int32_t)ei[n + i] : 0;
    } else {
      key[r] = valid ? keys_in[i] : 0xffffffffu;
      val[r] = valid ? vals_in[i] : 0u;
      tgt[r] = valid ? tgts_in[i] : 0;
    }
  }
  {  // where every digit starts: exclusive scan of the digit totals (its barriers cover the clearing)
    const uint32_t t = own ? digit_total[threadIdx.x] : 0u;
    const uint32_t ex = block_exclusive_scan(t, nullptr);
    if (own) dbase[threadIdx.x] = ex;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_ITEMS; ++r) {
    const int64_t i = wbase + r * 64 + lane;
    const bool valid = i < n;
    const uint32_t d = (key[r] >> shift) & mask;
    uint64_t peers = __ballot(valid);
    for (int b = 0; b < bits; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(valid && bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t pre = cnt[w][d];
    const uint32_t rk = __popcll(peers & lt);
    const uint32_t tot = __popcll(peers);
    rank[r] = pre + rk;
    __builtin_amdgcn_wave_barrier();
    if (valid && rk == tot - 1) cnt[w][d] = pre + tot;  // highest peer lane
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {  // per digit: the waves' offsets inside it, its first slot in the tile, destination - slot
    uint32_t tc = 0;
    if (own) {
#pragma unroll
      for (int w2 = 0; w2 < SORT_WAVES; ++w2) {
        const uint32_t t = cnt[w2][threadIdx.x];
        cnt[w2][threadIdx.x] = tc;
        tc += t;
      }
    }
    const uint32_t ex = block_exclusive_scan(tc, nullptr);
    if (own) {
      texcl[threadIdx.x] = ex;
      dbase[threadIdx.x] += blockoff[(size_t)threadIdx.x * nblocks + blockIdx.x] - ex;   // (mod 2^32)
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_ITEMS; ++r) {   // every element's slot, before the counters' words are reused
    const uint32_t d = (key[r] >> shift) & mask;
    rank[r] += texcl[d] + cnt[w][d];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_ITEMS; ++r) {
    const int64_t i = wbase + r * 64 + lane;
    if (i < n) {
      buf[rank[r]] = key[r];
      buf[SORT_TILE + rank[r]] = val[r];
      buf[2 * SORT_TILE + rank[r]] = (uint32_t)tgt[r];
    }
  }
  __syncthreads();
  const int tn = (int)((n - tbase) < (int64_t)SORT_TILE ? (n - tbase) : (int64_t)SORT_TILE);
  for (int j = threadIdx.x; j < tn; j += SORT_THREADS) {
    const uint32_t k = buf[j];
    const uint32_t v = buf[SORT_TILE + j];
    const uint32_t dst = dbase[(k >> shift) & mask] + (uint32_t)j;
    keys_out[dst] = k;
    vals_out[dst] = v;
    tgts_out[dst] = (int32_t)buf[2 * SORT_TILE + j];
    if constexpr (LAST)
      if (inv) inv[v] = (int32_t)dst;
  }
}

}  // namespace spt
