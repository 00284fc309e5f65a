// CSR view of an unsorted segment index: stable LSD radix sort of (idx, iota)
// followed by boundary detection.  Hand-written for gfx950 (wave64 ballots for
// the stable in-wave ranking; 4-wave workgroups; LDS digit counters).
//
// Why a sort at all: the reference groups rows by index with float atomics in
// torch_scatter's COO kernels on every call (src/nn/pool.py:61-62,
// src/nn/norm.py:118-126, src/nn/attention.py:307,315).  We group ONCE per
// batch and level, deterministically, and every later segment kernel streams
// rows through (perm, rowptr) without atomics.
#include "radix_sort.hpp"

using namespace spt;

extern "C" size_t spt_csr_build_workspace_bytes(int64_t n, int64_t num_seg) {
  if (n < 0 || num_seg < 1) return 0;
  return RadixScratch::bytes(n);
}

extern "C" int spt_csr_build(const int64_t* idx, int64_t n, int64_t num_seg,
                             int32_t* perm, int32_t* rowptr, void* ws,
                             size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31) - SORT_TILE, "n out of range");
  SPT_CHECK_ARG(num_seg >= 1 && num_seg < ((int64_t)1 << 31), "num_seg out of range");
  SPT_CHECK_ARG(rowptr != nullptr, "rowptr is null");
  SPT_CHECK_ARG(n == 0 || (idx && perm), "null idx/perm");
  const size_t need = RadixScratch::bytes(n);
  SPT_CHECK_ARG(ws_bytes >= need && (ws || need == 0), "workspace too small");

  if (n == 0) {
    rowptr_from_sorted_kernel<<<stream_grid(num_seg + 1, 256), 256, 0, stream>>>(
        nullptr, 0, num_seg, rowptr);
    SPT_CHECK_LAUNCH();
    return 0;
  }
  if (num_seg <= 1) {
    iota_kernel<<<stream_grid(n, 256), 256, 0, stream>>>(perm, n);
    rowptr_single_kernel<<<1, 1, 0, stream>>>(rowptr, n);
    SPT_CHECK_LAUNCH();
    return 0;
  }
  RadixScratch s;
  s.carve((char*)ws, n);
  const uint32_t *ks, *vs;
  SPT_CHECK_ARG(radix_sort_pairs<1>(idx, nullptr, nullptr, n, bits_for(num_seg), s,
                                    (uint32_t*)perm, &ks, &vs, stream) == 0,
                "scan partials do not fit their region");
  rowptr_from_sorted_kernel<<<stream_grid(n + 1, 256), 256, 0, stream>>>(
      ks, n, num_seg, rowptr);
  SPT_CHECK_LAUNCH();
  return 0;
}


// ---- companions of the CSR view the host side otherwise builds with torch gathers ------------
namespace spt {
// pos_seg[j] = the segment of CSR position j (= idx[perm[j]], without touching idx: segment s
// owns positions rowptr[s] .. rowptr[s + 1]).  One lane group of 16 per segment (segments of the
// L0 -> L1 pool hold ~35 rows), coalesced stores.
__global__ __launch_bounds__(256) void csr_pos_seg_kernel(const int32_t* __restrict__ rowptr,
                                                          int64_t num_seg,
                                                          int32_t* __restrict__ pos_seg) {
  const int sub = threadIdx.x & 15;
  const int64_t stride = (int64_t)gridDim.x * 16;
  for (int64_t s = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); s < num_seg; s += stride) {
    const int a = rowptr[s], b = rowptr[s + 1];
    for (int j = a + sub; j < b; j += 16) pos_seg[j] = (int32_t)s;
  }
}
// out[j] = (int32) src[perm[j]]: e.g. the targets of the edges in CSR order
__global__ __launch_bounds__(256) void csr_gather_i64_i32_kernel(const int64_t* __restrict__ src,
                                                                 const int32_t* __restrict__ perm,
                                                                 int64_t n, int32_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride)
    out[j] = (int32_t)src[perm[j]];
}
}  // namespace spt

extern "C" int spt_csr_pos_seg(const int32_t* rowptr, int64_t num_seg, int64_t n, int32_t* pos_seg,
                               spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(num_seg >= 0 && n >= 0, "bad shape");
  if (n == 0 || num_seg == 0) return 0;
  SPT_CHECK_ARG(rowptr && pos_seg, "null pointer");
  spt::csr_pos_seg_kernel<<<spt::stream_grid(num_seg, 16), 256, 0, stream>>>(rowptr, num_seg, pos_seg);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_csr_gather_i64_i32(const int64_t* src, const int32_t* perm, int64_t n,
                                      int32_t* out, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(n >= 0, "bad shape");
  if (n == 0) return 0;
  SPT_CHECK_ARG(src && perm && out, "null pointer");
  spt::csr_gather_i64_i32_kernel<<<spt::stream_grid(n, 256), 256, 0, stream>>>(src, perm, n, out);
  SPT_CHECK_LAUNCH();
  return 0;
}


// ---- the edge view of an attention graph in one entry --------------------------------------------
// Stable sort of the edges by source (radix_sort.hpp, "the edge sort"), the last pass writing the
// tables a level's attention calls read - eperm, src_sorted, tgt_sorted, inv - then erowptr from
// the sorted sources and, for a list whose maker declared the mirror structure
// [i<j | j>i | loops], its check (riding on the first read of the sources) and the target-order
// tile records.  Launches: hist, row scan, scatter per pass, + row pointers, + records: 11 for
// the three passes of 17 .. 24 key bits, 8 for two passes.
#include "edge_attn_internal.hpp"

namespace spt {
struct EdgeCsrPlan {
  int nblocks;
  size_t off_k[2], off_v[2], off_t[2], off_hist, off_tot, off_bad, total;
};
// two (key, value, target) scratch triples (passes ping-pong, the last writes the tables), the
// histograms [digit][workgroup] of one pass, the digit totals, one verdict word per workgroup.
// The row scan needs no partials region.
static inline EdgeCsrPlan edge_csr_plan(int64_t e) {
  EdgeCsrPlan p;
  const int64_t m = e > 0 ? e : 1;
  p.nblocks = (int)ceil_div(m, SORT_TILE);
  const size_t nb = align_up((size_t)m * 4, 256);
  size_t o = 0;
  for (int i = 0; i < 2; ++i) {
    p.off_k[i] = o; o += nb;
    p.off_v[i] = o; o += nb;
    p.off_t[i] = o; o += nb;
  }
  p.off_hist = o; o += align_up((size_t)MAX_BINS * p.nblocks * 4, 256);
  p.off_tot = o;  o += align_up((size_t)MAX_BINS * 4, 256);
  p.off_bad = o;  o += align_up((size_t)p.nblocks * 4, 256);
  p.total = o;
  return p;
}
}  // namespace spt

extern "C" size_t spt_edge_csr_build_workspace_bytes(int64_t e, int64_t n) {
  if (e < 0 || n < 1) return 0;
  return spt::edge_csr_plan(e).total;
}

extern "C" int spt_edge_csr_build(const int64_t* edge_index, int64_t e, int64_t n, int64_t pairs,
                                  int32_t* erowptr, int32_t* eperm, int32_t* tgt_sorted,
                                  int32_t* src_sorted, int32_t* inv, int32_t* tile_ids,
                                  int32_t* flag, void* ws, size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(e >= 1 && e < ((int64_t)1 << 31) - SORT_TILE, "e out of range");
  SPT_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "n out of range");
  SPT_CHECK_ARG(pairs >= -1 && 2 * pairs <= e, "bad mirror count");
  SPT_CHECK_ARG(edge_index && erowptr && eperm && tgt_sorted && src_sorted && flag, "null pointer");
  SPT_CHECK_ARG(pairs >= 0 || !tile_ids, "tile records need a mirror count");
  SPT_CHECK_ARG(!tile_ids || inv, "tile records need inv");
  const EdgeCsrPlan p = edge_csr_plan(e);
  SPT_CHECK_ARG(ws && ws_bytes >= p.total, "workspace too small");
  char* w = (char*)ws;
  uint32_t* kbuf[2] = {(uint32_t*)(w + p.off_k[0]), (uint32_t*)(w + p.off_k[1])};
  uint32_t* vbuf[2] = {(uint32_t*)(w + p.off_v[0]), (uint32_t*)(w + p.off_v[1])};
  int32_t* tbuf[2] = {(int32_t*)(w + p.off_t[0]), (int32_t*)(w + p.off_t[1])};
  uint32_t* hist = (uint32_t*)(w + p.off_hist);
  uint32_t* tot = (uint32_t*)(w + p.off_tot);
  uint32_t* bad = (uint32_t*)(w + p.off_bad);

  const int nbits = bits_for(n);
  const int passes = (nbits + 7) / 8;
  const int per = (nbits + passes - 1) / passes;      // balanced digits, e.g. 19 -> 7 + 6 + 6
  const int nblocks = p.nblocks;
  const uint32_t* kin = nullptr;
  const uint32_t* vin = nullptr;
  const int32_t* tin = nullptr;
  int shift = 0;
  for (int pass = 0; pass < passes; ++pass) {
    const int bits = (nbits - shift < per) ? (nbits - shift) : per;
    const bool last = pass == passes - 1;
    uint32_t* kout = last ? (uint32_t*)src_sorted : kbuf[pass & 1];
    uint32_t* vout = last ? (uint32_t*)eperm : vbuf[pass & 1];
    int32_t* tout = last ? tgt_sorted : tbuf[pass & 1];
    if (pass == 0)
      edge_hist_kernel<true><<<nblocks, SORT_THREADS, 0, stream>>>(
          edge_index, nullptr, e, shift, bits, hist, nblocks, pairs, bad);
    else
      edge_hist_kernel<false><<<nblocks, SORT_THREADS, 0, stream>>>(
          nullptr, kin, e, shift, bits, hist, nblocks, -1, nullptr);
    edge_rowscan_kernel<<<1 << bits, SCAN_THREADS, 0, stream>>>(hist, nblocks, tot, bad,
                                                               pass == 0 ? flag : nullptr);
    if (pass == 0 && last)
      edge_scatter_kernel<1, true><<<nblocks, SORT_THREADS, 0, stream>>>(
          edge_index, nullptr, nullptr, nullptr, e, shift, bits, hist, tot, nblocks, kout, vout, tout, inv);
    else if (pass == 0)
      edge_scatter_kernel<1, false><<<nblocks, SORT_THREADS, 0, stream>>>(
          edge_index, nullptr, nullptr, nullptr, e, shift, bits, hist, tot, nblocks, kout, vout, tout, nullptr);
    else if (last)
      edge_scatter_kernel<0, true><<<nblocks, SORT_THREADS, 0, stream>>>(
          nullptr, kin, vin, tin, e, shift, bits, hist, tot, nblocks, kout, vout, tout, inv);
    else
      edge_scatter_kernel<0, false><<<nblocks, SORT_THREADS, 0, stream>>>(
          nullptr, kin, vin, tin, e, shift, bits, hist, tot, nblocks, kout, vout, tout, nullptr);
    kin = kout;
    vin = vout;
    tin = tout;
    shift += bits;
  }
  rowptr_from_sorted_kernel<<<stream_grid(e + 1, 256), 256, 0, stream>>>(
      (const uint32_t*)src_sorted, e, n, erowptr);
  if (tile_ids)
    attn_pack_tile_ids_mirror_launch(eperm, tgt_sorted, src_sorted, inv, e, pairs, tile_ids, stream);
  SPT_CHECK_LAUNCH();
  return 0;
}
