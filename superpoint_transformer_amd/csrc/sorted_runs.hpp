// Wide-key grouping: "sort keys wider than one 32-bit word, find the runs of equal keys".
// Shared by voxel.hip, panoptic.hip, sparse_conv.hip, merge.hip and cluster_graph.hip; sits on
// the pair sort and the device scan of radix_sort.hpp.
//
// A key is (major, minor): two u32 words of major_bits and minor_bits bits, ordered by the major
// word first.  major_bits == 0 is a key of one word, kept in the minor word's place.  The sort
// is two stable LSD radix sorts - by the minor word, a gather of the major word through that
// permutation, by the major word - and returns the permutation `order` and the sorted major (or
// only) word.  The key of sorted position i is then sorted_key(): the sorted major word and the
// minor word of element order[i].
//
// Runs.  flag[i] = 1 where a run of equal keys starts, flag[n] = 0; after the exclusive scan
// flag[i + 1] - 1 is the run of sorted position i and flag[n] the number of runs R.
// run_start[r] is the first sorted position of run r.  `limit` is an exclusive upper bound on
// the major word: sorted positions at or above it are the rejected tail - they head no run and
// run_start[R] is the first of them (n when there is none).  NO_MAJOR_LIMIT rejects nothing.
//
// Every host function returns 0, or -1 when a scratch region is too small for a step; nothing
// of that step is launched.  Callers put their own message on the result.
#pragma once
#include "radix_sort.hpp"

namespace spt {

constexpr int RUNS_THREADS = 256;
constexpr uint64_t NO_MAJOR_LIMIT = 1ull << 32;       // above every major word

static __global__ void gather_u32_kernel(const uint32_t* __restrict__ src,
                                         const uint32_t* __restrict__ perm, int64_t n,
                                         uint32_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = src[perm[i]];
}

// ---- the sort ------------------------------------------------------------------------------------
// Scratch: the minor word [n], and for two words the major word [n + 1], its gathered copy [n];
// then the pair sort's own scratch, where `order` and the sorted word end up.  The major region
// has one word more than the keys need so that run starts [R + 1] fit over it (RunsPlan).
struct SortPlan {
  size_t off_minor, off_major, off_gmaj, off_sort, total;
  int minor_bits, major_bits;
};

static inline SortPlan sort_plan(int64_t n, int minor_bits, int major_bits) {
  SortPlan p;
  const size_t nb = align_up((size_t)(n > 0 ? n : 1) * 4, 256);
  const bool two = major_bits > 0;
  size_t off = 0;
  p.off_minor = off; off += nb;
  p.off_major = off; off += two ? align_up((size_t)(n + 1) * 4, 256) : 0;
  p.off_gmaj = off; off += two ? nb : 0;
  p.off_sort = off; off += RadixScratch::bytes(n);
  p.total = off;
  p.minor_bits = minor_bits;
  p.major_bits = major_bits;
  return p;
}

// a key of key_bits bits, the low 32 of them in the minor word
static inline SortPlan sort_plan(int64_t n, int key_bits) {
  return sort_plan(n, key_bits > 32 ? 32 : key_bits, key_bits > 32 ? key_bits - 32 : 0);
}

// where the caller writes its keys (major: null for one word)
struct WideKeys {
  uint32_t *minor, *major;
};

static inline WideKeys sort_carve(char* base, const SortPlan& p) {
  WideKeys k;
  k.minor = (uint32_t*)(base + p.off_minor);
  k.major = p.major_bits > 0 ? (uint32_t*)(base + p.off_major) : nullptr;
  return k;
}

// what the sort leaves: the sorted major (or only) word, the UNSORTED minor word (null for one
// word) and the permutation
struct SortedKeys {
  const uint32_t *major, *minor, *order;
};

__device__ __forceinline__ uint64_t sorted_key(const SortedKeys& k, int64_t i) {
  if (!k.minor) return k.major[i];
  return ((uint64_t)k.major[i] << 32) | k.minor[k.order[i]];
}

// Stable sort of the n keys at sort_carve(base, p).  The second sort's first pass writes the
// scratch's value buffers, so the first sort's permutation must live outside them: `perm` is n
// words the caller lends for the time of the call (not used for one word).
static inline int sort_wide(char* base, const SortPlan& p, int64_t n, uint32_t* perm,
                            hipStream_t stream, SortedKeys* out) {
  const WideKeys k = sort_carve(base, p);
  RadixScratch s;
  s.carve(base + p.off_sort, n);
  out->minor = k.major ? k.minor : nullptr;
  if (!k.major)
    return radix_sort_pairs<2>(nullptr, k.minor, nullptr, n, p.minor_bits, s, nullptr,
                               &out->major, &out->order, stream);
  const uint32_t *ks = nullptr, *vs = nullptr;
  if (radix_sort_pairs<2>(nullptr, k.minor, nullptr, n, p.minor_bits, s, perm, &ks, &vs, stream))
    return -1;
  uint32_t* gmaj = (uint32_t*)(base + p.off_gmaj);
  gather_u32_kernel<<<stream_grid(n, RUNS_THREADS), RUNS_THREADS, 0, stream>>>(k.major, perm, n,
                                                                               gmaj);
  return radix_sort_pairs<0>(nullptr, gmaj, perm, n, p.major_bits, s, nullptr, &out->major,
                             &out->order, stream);
}

// ---- the runs ------------------------------------------------------------------------------------
static __global__ void run_heads_kernel(SortedKeys k, int64_t n, uint64_t limit,
                                        uint32_t* __restrict__ flag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) {
    uint32_t f = 0;
    if (i < n && k.major[i] < limit)
      f = (i == 0) || sorted_key(k, i) != sorted_key(k, i - 1);
    flag[i] = f;
  }
}

static __global__ void run_starts_kernel(const uint32_t* __restrict__ smajor,
                                         const uint32_t* __restrict__ excl, int64_t n,
                                         uint64_t limit, int32_t* __restrict__ run_start) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool all = limit > 0xffffffffull;                       // no limit: the words are not read
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) {
    const bool kept = i < n && (all || smajor[i] < limit);
    const bool prev_kept = i > 0 && (all || smajor[i - 1] < limit);
    if (kept && excl[i + 1] != excl[i]) run_start[excl[i]] = (int32_t)i;   // excl[i] < R <= n
    if (!kept && (i == 0 || prev_kept)) run_start[excl[n]] = (int32_t)i;   // the tail, or n
  }
}

// Scratch of sort + runs: the sort's, the flag array [n + 1] with its scan partials, and (when
// asked for) the run starts [n + 1].  With two words the starts lie over the unsorted major
// word, which is dead once gathered: a caller that wants run starts does not read it again.
struct RunsPlan {
  SortPlan sort;
  ScanPlan scan;
  size_t off_scan, off_start, total;
};

static inline RunsPlan runs_plan(int64_t n, int minor_bits, int major_bits, bool starts) {
  RunsPlan p;
  p.sort = sort_plan(n, minor_bits, major_bits);
  p.scan = scan_plan(n + 1);
  size_t off = p.sort.total;
  p.off_scan = off; off += p.scan.total;
  p.off_start = major_bits > 0 ? p.sort.off_major : off;
  if (starts && major_bits == 0) off += align_up((size_t)(n + 1) * 4, 256);
  p.total = off;
  return p;
}

static inline RunsPlan runs_plan(int64_t n, int key_bits, bool starts) {
  return runs_plan(n, key_bits > 32 ? 32 : key_bits, key_bits > 32 ? key_bits - 32 : 0, starts);
}

struct Runs {
  WideKeys in;                 // the keys, written by the caller
  SortedKeys sorted;           // after the sort
  uint32_t* excl;              // [n + 1]: flags, then their exclusive scan
  const uint32_t* num_runs;    // = excl + n
  int32_t* run_start;          // [R + 1] (a plan with starts)
};

static inline Runs runs_carve(char* base, const RunsPlan& p, int64_t n) {
  Runs r;
  r.in = sort_carve(base, p.sort);
  r.sorted = SortedKeys{nullptr, nullptr, nullptr};
  r.excl = (uint32_t*)(base + p.off_scan);
  r.num_runs = r.excl + n;
  r.run_start = (int32_t*)(base + p.off_start);
  return r;
}

// the sort of a runs plan: the flag array is dead until the heads are flagged and holds the
// first sort's permutation meanwhile
static inline int sort_runs(char* base, const RunsPlan& p, Runs& r, int64_t n,
                            hipStream_t stream) {
  return sort_wide(base, p.sort, n, r.excl, stream, &r.sorted);
}

// flags of the sorted keys and their exclusive scan
static inline int flag_runs(char* base, const RunsPlan& p, const Runs& r, int64_t n,
                            uint64_t limit, hipStream_t stream) {
  if (scan_part_entries(n + 1) > p.scan.part_cap) return -1;
  run_heads_kernel<<<stream_grid(n + 1, RUNS_THREADS), RUNS_THREADS, 0, stream>>>(r.sorted, n,
                                                                                  limit, r.excl);
  uint32_t* part = (uint32_t*)(base + p.off_scan + p.scan.off_part);
  return device_exclusive_scan(r.excl, n + 1, part, p.scan.part_cap, stream);
}

// r.in holds the keys: stable sort, heads, scan, run starts
static inline int find_runs(char* base, const RunsPlan& p, Runs& r, int64_t n, uint64_t limit,
                            hipStream_t stream) {
  if (sort_runs(base, p, r, n, stream)) return -1;
  if (flag_runs(base, p, r, n, limit, stream)) return -1;
  run_starts_kernel<<<stream_grid(n + 1, RUNS_THREADS), RUNS_THREADS, 0, stream>>>(
      r.sorted.major, r.excl, n, limit, r.run_start);
  return 0;
}

}  // namespace spt
