// Edge-contrast focal loss of the partition training stage (PartitionCriterion,
// src/loss/partition_criterion.py:92-145, with BinaryFocalLoss, src/loss/focal.py:194-220).
//
// The reference compacts the edge list three times with boolean masks, reads the number of
// inter-edges back, draws its sample with a host-sized randperm and back-propagates through two
// atomic index_adds.  Here nothing is compacted and nothing is read back:
//
//   node pass      label[n] = first arg-max of y[n, :C], -1 for a void node (max == 0)
//   classify       code[e] = 0 dropped (self loop, a void end, an end outside [0, N)), 1 inter,
//                  2 intra; the three counters by integer atomics (any order, same sum)
//   plan           n_major = (int) (f32(n_inter) * f32(1 / ratio - 1)), clamped to n_intra
//   radix select   the n_major-th smallest key (rand32(s, e) << 32 | e) of the intra edges: six
//                  passes of an 11-bit histogram (the last one 9 bits) and a one-workgroup scan.
//                  The keys are distinct, so "key <= K" selects exactly n_major edges and a tie
//                  of two draws goes to the lower e.
//   loss           eight lanes per edge, selected edges only: d, p, q, q', l in f64; f64 partial
//                  sums per workgroup, added in a fixed order by the finish kernel, which also
//                  takes the "no edge / no inter edge -> 0" decision from the device counters and
//                  advances the call counter of `state`
//   backward       eight lanes per NODE walk the node's run of the by-source view, then of the
//                  by-target view (stable: ascending edge position) and write the row once.
//
// No float atomics anywhere: every output is bitwise reproducible.
#include "common.hpp"
#include "rng.hpp"

namespace spt {

constexpr int PL_BLOCK = 256;
constexpr int PL_LANES = 8;                         // lanes per edge / node
constexpr int PL_GROUPS = PL_BLOCK / PL_LANES;      // 32 edges / nodes per workgroup and step
constexpr int PL_STEPS = 16;                        // steps of the loss kernel per workgroup
constexpr int PL_EDGES = PL_GROUPS * PL_STEPS;      // 512 edges per workgroup of the loss kernel
constexpr int PL_MAXD = 128;
constexpr int PL_BINS = 2048;                       // 11-bit digits
constexpr int PL_PASSES = 6;                        // 5 x 11 + 9 = 64 bits

// control block at the head of the workspace (int64 each)
enum { CTL_INTER = 0, CTL_INTRA, CTL_BAD, CTL_MAJOR, CTL_PREFIX, CTL_REM, CTL_SEED, CTL_MODE, CTL_CLAMP,
       CTL_WORDS = 16 };
enum { MODE_NONE = 0, MODE_ALL = 1, MODE_SELECT = 2 };

constexpr size_t PL_CTL_BYTES = 256;
constexpr size_t PL_HIST_BYTES = PL_BINS * sizeof(uint32_t);

__host__ __device__ __forceinline__ int pl_shift(int pass) { return pass < 5 ? 53 - 11 * pass : 0; }
__host__ __device__ __forceinline__ int pl_width(int pass) { return pass < 5 ? 11 : 9; }

// the stream of call number `calls`: two draws of the package's generator make the 64-bit mask
__host__ __device__ __forceinline__ uint64_t pl_call_seed(uint64_t seed, uint64_t calls) {
  const uint64_t hi = rand32(0x5EEDull, 2 * calls), lo = rand32(0x5EEDull, 2 * calls + 1);
  return seed ^ ((hi << 32) | lo);
}

__device__ __forceinline__ uint64_t pl_key(uint64_t s, int64_t e) {
  return ((uint64_t)rand32(s, (uint64_t)e) << 32) | (uint64_t)(uint32_t)e;
}

__global__ __launch_bounds__(PL_BLOCK) void pl_label_kernel(const int64_t* __restrict__ y, int ycols,
                                                           int C, int64_t N,
                                                           int32_t* __restrict__ label) {
  const int64_t n = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x;
  if (n >= N) return;
  int lab = -1;
  if (ycols == 0) {                                 // label vector: [0, C) is a class, the rest void
    const int64_t v = y[n];
    if (v >= 0 && v < C) lab = (int)v;
  } else {
    const int64_t* h = y + n * ycols;
    int64_t best = h[0];
    lab = 0;
    for (int c = 1; c < C; ++c) {
      const int64_t v = h[c];
      if (v > best) {                               // strict: ties to the lowest label
        best = v;
        lab = c;
      }
    }
    if (best == 0) lab = -1;
  }
  label[n] = lab;
}

__global__ __launch_bounds__(PL_BLOCK) void pl_classify_kernel(
    const int64_t* __restrict__ ei, int64_t E, int64_t N, const int32_t* __restrict__ label,
    uint8_t* __restrict__ code, int64_t* __restrict__ ctl) {
  __shared__ int s_n[3][PL_BLOCK / 64];
  const int64_t e = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x;
  int c = 0, bad = 0;
  if (e < E) {
    const int64_t i = ei[e], j = ei[E + e];
    if (i < 0 || i >= N || j < 0 || j >= N) {       // compared with the bound before it indexes
      bad = 1;
    } else if (i != j) {
      const int li = label[i], lj = label[j];
      if (li >= 0 && lj >= 0) c = (li == lj) ? 2 : 1;
    }
    code[e] = (uint8_t)c;
  }
  const int wave = threadIdx.x >> 6;
  const int n1 = __popcll(__ballot(c == 1)), n2 = __popcll(__ballot(c == 2)),
            nb = __popcll(__ballot(bad));
  if ((threadIdx.x & 63) == 0) {
    s_n[0][wave] = n1;
    s_n[1][wave] = n2;
    s_n[2][wave] = nb;
  }
  __syncthreads();
  if (threadIdx.x < 3) {                            // integer sums: any arrival order gives the same
    int n = 0;
    for (int w = 0; w < PL_BLOCK / 64; ++w) n += s_n[threadIdx.x][w];
    if (n) atomicAdd(reinterpret_cast<unsigned long long*>(ctl) + threadIdx.x, (unsigned long long)n);
  }
}

// one thread: how many intra edges the sample keeps and how the later kernels find them
__global__ void pl_plan_kernel(int64_t* __restrict__ ctl, int sampling, float major_per_inter,
                               const int64_t* __restrict__ state) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t n_inter = ctl[CTL_INTER], n_intra = ctl[CTL_INTRA];
  int64_t n_major = n_intra, clamp = 0;
  if (sampling) {
    // torch's ((1 / r - 1) * count).int(): the product of two f32, truncated
    const float prod = (float)n_inter * major_per_inter;
    n_major = prod >= 9.2e18f ? INT64_MAX : (int64_t)prod;
    if (n_major < 0) n_major = 0;
    if (n_major > n_intra) {                        // the reference asserts here
      n_major = n_intra;
      clamp = 1;
    }
  }
  ctl[CTL_MAJOR] = n_major;
  ctl[CTL_PREFIX] = 0;
  ctl[CTL_REM] = n_major;
  ctl[CTL_CLAMP] = clamp;
  ctl[CTL_MODE] = n_major == 0 ? MODE_NONE : (n_major == n_intra ? MODE_ALL : MODE_SELECT);
  ctl[CTL_SEED] = state ? (int64_t)pl_call_seed((uint64_t)state[0], (uint64_t)state[1]) : 0;
}

__global__ __launch_bounds__(PL_BLOCK) void pl_hist_kernel(const uint8_t* __restrict__ code, int64_t E,
                                                          const int64_t* __restrict__ ctl, int pass,
                                                          uint32_t* __restrict__ hist) {
  if (ctl[CTL_MODE] != MODE_SELECT) return;         // uniform: nothing to select
  __shared__ uint32_t s_h[PL_BINS];
  for (int i = threadIdx.x; i < PL_BINS; i += PL_BLOCK) s_h[i] = 0u;
  __syncthreads();
  const uint64_t seed = (uint64_t)ctl[CTL_SEED], prefix = (uint64_t)ctl[CTL_PREFIX];
  const int shift = pl_shift(pass), width = pl_width(pass);
  const uint32_t mask = (1u << width) - 1u;
  for (int64_t e = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x; e < E;
       e += (int64_t)gridDim.x * PL_BLOCK) {
    if (code[e] != 2) continue;
    const uint64_t key = pl_key(seed, e);
    if (pass > 0 && (key >> (shift + width)) != prefix) continue;
    atomicAdd(&s_h[(uint32_t)(key >> shift) & mask], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < PL_BINS; i += PL_BLOCK)
    if (s_h[i]) atomicAdd(&hist[i], s_h[i]);
}

// one workgroup: the digit of this pass that holds the key of rank `rem`; clears the histogram
__global__ __launch_bounds__(PL_BLOCK) void pl_scan_kernel(int64_t* __restrict__ ctl, int pass,
                                                          uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_h[PL_BINS];
  for (int i = threadIdx.x; i < PL_BINS; i += PL_BLOCK) {
    s_h[i] = hist[i];
    hist[i] = 0u;
  }
  __syncthreads();
  if (threadIdx.x != 0 || ctl[CTL_MODE] != MODE_SELECT) return;
  const int nbins = 1 << pl_width(pass);
  const int64_t rem = ctl[CTL_REM];
  int64_t cum = 0;
  int digit = nbins - 1;
  for (int b = 0; b < nbins; ++b) {
    if (cum + (int64_t)s_h[b] >= rem) {
      digit = b;
      break;
    }
    cum += s_h[b];
  }
  ctl[CTL_PREFIX] = (int64_t)(((uint64_t)ctl[CTL_PREFIX] << pl_width(pass)) | (uint64_t)digit);
  ctl[CTL_REM] = rem - cum;
}

// four consecutive floats of a row from column `col`, zero past D
__device__ __forceinline__ float4 pl_load4(const float* __restrict__ row, int col, int D, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec) {
    if (col < D) v = *reinterpret_cast<const float4*>(row + col);
  } else {
    if (col < D) v.x = row[col];
    if (col + 1 < D) v.y = row[col + 1];
    if (col + 2 < D) v.z = row[col + 2];
    if (col + 3 < D) v.w = row[col + 3];
  }
  return v;
}

__device__ __forceinline__ double pl_group_sum(double v) {   // over the 8 lanes of a group
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

struct FocalParams {
  double inv_t, gamma, weight, eps;
};

// q' of an edge at distance d and its p
__device__ __forceinline__ double pl_qprime(bool intra, double d, const FocalParams& f, double* p_out) {
  const double p = exp(-d * f.inv_t);
  *p_out = p;
  const double q = intra ? p : 1.0 - p;
  return f.eps + (1.0 - 2.0 * f.eps) * q;
}

__device__ __forceinline__ double pl_term(bool intra, double d, const FocalParams& f) {
  double p;
  const double qp = pl_qprime(intra, d, f, &p);
  const double w = intra ? f.weight : 1.0 - f.weight;
  const double mod = f.gamma == 0.0 ? 1.0 : pow(1.0 - qp, f.gamma);
  return -w * mod * log(qp);
}

// c_e = dl/dd / d (0 at d == 0, torch's norm backward)
__device__ __forceinline__ double pl_coef(bool intra, double d, const FocalParams& f) {
  if (!(d > 0.0)) return 0.0;
  double p;
  const double qp = pl_qprime(intra, d, f, &p);
  const double w = intra ? f.weight : 1.0 - f.weight;
  const double one_m = 1.0 - qp;
  double dl_dq;
  if (f.gamma == 0.0) {
    dl_dq = -1.0 / qp;
  } else {
    dl_dq = f.gamma * pow(one_m, f.gamma - 1.0) * log(qp) - pow(one_m, f.gamma) / qp;
  }
  const double sign = intra ? 1.0 : -1.0;
  return w * dl_dq * (1.0 - 2.0 * f.eps) * sign * (-p * f.inv_t) / d;
}

template <int NCH>
__global__ __launch_bounds__(PL_BLOCK) void pl_loss_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t N, int D, bool vec,
    const int64_t* __restrict__ ei, int64_t E, uint8_t* __restrict__ code,
    const int64_t* __restrict__ ctl, FocalParams f, uint8_t* __restrict__ selected,
    double* __restrict__ partial) {
  __shared__ double s_sum[PL_GROUPS];
  const int group = threadIdx.x / PL_LANES, lane = threadIdx.x % PL_LANES;
  const int mode = (int)ctl[CTL_MODE];
  const uint64_t seed = (uint64_t)ctl[CTL_SEED], kth = (uint64_t)ctl[CTL_PREFIX];
  double sum = 0.0;
  const int64_t base = (int64_t)blockIdx.x * PL_EDGES;
  for (int step = 0; step < PL_STEPS; ++step) {
    const int64_t e = base + (int64_t)step * PL_GROUPS + group;
    if (e >= E) break;                               // uniform over the group
    const int c = code[e];
    bool sel = c == 1;
    if (c == 2) sel = mode == MODE_ALL || (mode == MODE_SELECT && pl_key(seed, e) <= kth);
    if (lane == 0) {
      if (c == 2 && !sel) code[e] = 0;               // the backward reads the final choice
      if (selected) selected[e] = sel ? 1 : 0;
    }
    if (!sel) continue;                              // no row of an unselected edge is fetched
    const float* ri = x + ei[e] * ldx;
    const float* rj = x + ei[E + e] * ldx;
    double ss = 0.0;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int col = ch * 32 + lane * 4;
      const float4 a = pl_load4(ri, col, D, vec), b = pl_load4(rj, col, D, vec);
      const double d0 = (double)a.x - (double)b.x, d1 = (double)a.y - (double)b.y,
                   d2 = (double)a.z - (double)b.z, d3 = (double)a.w - (double)b.w;
      ss += d0 * d0;
      ss += d1 * d1;
      ss += d2 * d2;
      ss += d3 * d3;
    }
    ss = pl_group_sum(ss);
    if (lane == 0) sum += pl_term(c == 2, sqrt(ss), f);
  }
  if (lane == 0) s_sum[group] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int g = 0; g < PL_GROUPS; ++g) a += s_sum[g];
    partial[blockIdx.x] = a;
  }
}

__global__ __launch_bounds__(256) void pl_finish_kernel(
    const double* __restrict__ partial, int nblocks, const int64_t* __restrict__ ctl,
    float* __restrict__ loss, double* __restrict__ den, int64_t* __restrict__ counts,
    int32_t* __restrict__ status, int64_t* __restrict__ state) {
  __shared__ double s_a[256];
  double a = 0.0;
  const int per = (nblocks + 255) / 256;
  const int lo = threadIdx.x * per, hi = (lo + per < nblocks) ? lo + per : nblocks;
  for (int i = lo; i < hi; ++i) a += partial[i];
  s_a[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int i = 0; i < 256; ++i) total += s_a[i];
  const int64_t n_inter = ctl[CTL_INTER], n_intra = ctl[CTL_INTRA];
  const int64_t n_sel = n_inter + ctl[CTL_MAJOR];
  // the reference's fake_edge_classification_loss: no kept edge or no inter edge
  const bool fake = n_inter == 0 || n_sel == 0;
  loss[0] = fake ? 0.f : (float)(total / (double)n_sel);
  den[0] = fake ? 0.0 : (double)n_sel;
  if (counts) {
    counts[0] = n_inter;
    counts[1] = n_intra;
    counts[2] = n_sel;
  }
  if (status) {
    const int64_t bad = ctl[CTL_BAD] > INT32_MAX ? INT32_MAX : ctl[CTL_BAD];
    status[0] += (int32_t)bad;
    status[1] |= (int32_t)ctl[CTL_CLAMP];
  }
  if (state) state[1] += 1;                          // the next call (or replay) draws afresh
}

template <int NCH>
__global__ __launch_bounds__(PL_BLOCK) void pl_bwd_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t N, int D, bool vec,
    const int64_t* __restrict__ ei, int64_t E, const uint8_t* __restrict__ code,
    const int32_t* __restrict__ src_rowptr, const int32_t* __restrict__ src_perm,
    const int32_t* __restrict__ tgt_rowptr, const int32_t* __restrict__ tgt_perm, FocalParams f,
    const float* __restrict__ gout, const double* __restrict__ den, float* __restrict__ gx,
    int64_t ldg, bool vec_out) {
  const int group = threadIdx.x / PL_LANES, lane = threadIdx.x % PL_LANES;
  const int64_t n = (int64_t)blockIdx.x * PL_GROUPS + group;
  if (n >= N) return;                                // uniform over the group
  const double dn = den[0];
  const double scale = dn > 0.0 ? (double)gout[0] / dn : 0.0;
  const float* rn = x + n * ldx;
  float4 own[NCH];
  double acc[NCH][4];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    own[ch] = pl_load4(rn, ch * 32 + lane * 4, D, vec);
    acc[ch][0] = acc[ch][1] = acc[ch][2] = acc[ch][3] = 0.0;
  }
  for (int side = 0; side < 2; ++side) {             // the runs as source, then as target
    const int32_t* rowptr = side == 0 ? src_rowptr : tgt_rowptr;
    const int32_t* perm = side == 0 ? src_perm : tgt_perm;
    const int64_t* other_end = side == 0 ? ei + E : ei;
    const int p0 = rowptr[n], p1 = rowptr[n + 1];
    for (int pos = p0; pos < p1; ++pos) {
      const int64_t e = perm[pos];
      if (e < 0 || e >= E) continue;                 // (a view that does not describe this list)
      const int c = code[e];
      if (c == 0) continue;
      const int64_t o = other_end[e];
      if (o < 0 || o >= N) continue;
      const float* ro = x + o * ldx;
      double diff[NCH][4];
      double ss = 0.0;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const float4 b = pl_load4(ro, ch * 32 + lane * 4, D, vec);
        diff[ch][0] = (double)own[ch].x - (double)b.x;
        diff[ch][1] = (double)own[ch].y - (double)b.y;
        diff[ch][2] = (double)own[ch].z - (double)b.z;
        diff[ch][3] = (double)own[ch].w - (double)b.w;
#pragma unroll
        for (int k = 0; k < 4; ++k) ss += diff[ch][k] * diff[ch][k];
      }
      ss = pl_group_sum(ss);
      const double ce = pl_coef(c == 2, sqrt(ss), f);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[ch][k] += ce * diff[ch][k];
    }
  }
  float* gr = gx + n * ldg;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int col = ch * 32 + lane * 4;
    const float4 g = make_float4((float)(scale * acc[ch][0]), (float)(scale * acc[ch][1]),
                                 (float)(scale * acc[ch][2]), (float)(scale * acc[ch][3]));
    if (vec_out) {
      if (col < D) *reinterpret_cast<float4*>(gr + col) = g;
    } else {
      if (col < D) gr[col] = g.x;
      if (col + 1 < D) gr[col + 1] = g.y;
      if (col + 2 < D) gr[col + 2] = g.z;
      if (col + 3 < D) gr[col + 3] = g.w;
    }
  }
}

static bool pl_sizes_ok(int64_t N, int64_t E, int D) {
  return N >= 1 && N < ((int64_t)1 << 31) && E >= 1 && E < ((int64_t)1 << 31) && D >= 1 &&
         D <= PL_MAXD;
}

static bool pl_params_ok(double temperature, double gamma, double weight, double epsilon) {
  return temperature > 0.0 && gamma >= 0.0 && weight >= 0.0 && weight <= 1.0 && epsilon >= 0.0 &&
         epsilon < 0.5;
}

static size_t pl_label_offset() { return PL_CTL_BYTES + PL_HIST_BYTES; }
static size_t pl_partial_offset(int64_t N) {
  return align_up(pl_label_offset() + (size_t)N * sizeof(int32_t), 256);
}

static bool pl_vec(const float* p, int64_t ld, int D) {
  return D % 4 == 0 && ld % 4 == 0 && aligned_to(p, 16);
}

}  // namespace spt

using namespace spt;

extern "C" size_t spt_partition_loss_workspace_bytes(int64_t N, int64_t E) {
  if (N < 1 || E < 1 || N >= ((int64_t)1 << 31) || E >= ((int64_t)1 << 31)) return 0;
  return pl_partial_offset(N) + (size_t)ceil_div(E, (int64_t)PL_EDGES) * sizeof(double);
}

extern "C" int spt_partition_loss_fwd_f32(
    const float* x, int64_t ldx, int64_t N, int D, const int64_t* y, int ycols, int C,
    const int64_t* edge_index, int64_t E, double temperature, double gamma, double weight,
    double epsilon, double ratio, int64_t* state, float* loss, double* den, uint8_t* code,
    int64_t* counts, int32_t* status, uint8_t* selected, void* ws, size_t ws_bytes,
    spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(D <= PL_MAXD, "rows wider than 128 features are not supported");
  SPT_CHECK_ARG(pl_sizes_ok(N, E, D), "1 <= N, E < 2^31 and 1 <= D <= 128");
  SPT_CHECK_ARG(ldx >= D, "row stride shorter than the row");
  SPT_CHECK_ARG(C >= 1 && (ycols == 0 || ycols >= C), "C >= 1 and y is [N] (ycols 0) or [N, >= C]");
  SPT_CHECK_ARG(pl_params_ok(temperature, gamma, weight, epsilon),
                "temperature > 0, gamma >= 0, weight in [0, 1], epsilon in [0, 0.5)");
  SPT_CHECK_ARG(ratio < 0.0 || (ratio > 0.0 && ratio <= 1.0), "ratio in (0, 1], or negative: no sampling");
  SPT_CHECK_ARG(ratio < 0.0 || state, "sampling needs the (seed, calls) state");
  SPT_CHECK_ARG(x && y && edge_index && loss && den && code, "null pointer");
  SPT_CHECK_ARG(aligned_to(x, 4) && aligned_to(y, 8) && aligned_to(edge_index, 8), "misaligned pointer");
  SPT_CHECK_ARG(ws && ws_bytes >= spt_partition_loss_workspace_bytes(N, E), "workspace too small");
  SPT_CHECK_ALIGNED(ws, 16);
  char* base = (char*)ws;
  int64_t* ctl = (int64_t*)base;
  uint32_t* hist = (uint32_t*)(base + PL_CTL_BYTES);
  int32_t* label = (int32_t*)(base + pl_label_offset());
  double* partial = (double*)(base + pl_partial_offset(N));
  const int sampling = ratio > 0.0 ? 1 : 0;
  const float major_per_inter = sampling ? (float)(1.0 / ratio - 1.0) : 0.f;
  const FocalParams f = {1.0 / temperature, gamma, weight, epsilon};
  const bool vec = pl_vec(x, ldx, D);
  const int nblocks = (int)ceil_div(E, (int64_t)PL_EDGES);

  if (hipMemsetAsync(base, 0, PL_CTL_BYTES + PL_HIST_BYTES, stream) != hipSuccess)
    return fail(-2, "%s: memset failed", __func__);
  pl_label_kernel<<<(int)ceil_div(N, (int64_t)PL_BLOCK), PL_BLOCK, 0, stream>>>(y, ycols, C, N, label);
  pl_classify_kernel<<<(int)ceil_div(E, (int64_t)PL_BLOCK), PL_BLOCK, 0, stream>>>(edge_index, E, N,
                                                                                  label, code, ctl);
  pl_plan_kernel<<<1, 64, 0, stream>>>(ctl, sampling, major_per_inter, sampling ? state : nullptr);
  if (sampling) {
    for (int pass = 0; pass < PL_PASSES; ++pass) {
      pl_hist_kernel<<<stream_grid(E, PL_BLOCK * 4), PL_BLOCK, 0, stream>>>(code, E, ctl, pass, hist);
      pl_scan_kernel<<<1, PL_BLOCK, 0, stream>>>(ctl, pass, hist);
    }
  }
  switch ((D + 31) / 32) {
    case 1: pl_loss_kernel<1><<<nblocks, PL_BLOCK, 0, stream>>>(x, ldx, N, D, vec, edge_index, E, code, ctl, f, selected, partial); break;
    case 2: pl_loss_kernel<2><<<nblocks, PL_BLOCK, 0, stream>>>(x, ldx, N, D, vec, edge_index, E, code, ctl, f, selected, partial); break;
    case 3: pl_loss_kernel<3><<<nblocks, PL_BLOCK, 0, stream>>>(x, ldx, N, D, vec, edge_index, E, code, ctl, f, selected, partial); break;
    default: pl_loss_kernel<4><<<nblocks, PL_BLOCK, 0, stream>>>(x, ldx, N, D, vec, edge_index, E, code, ctl, f, selected, partial); break;
  }
  pl_finish_kernel<<<1, 256, 0, stream>>>(partial, nblocks, ctl, loss, den, counts, status,
                                          sampling ? state : nullptr);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" int spt_partition_loss_bwd_f32(
    const float* x, int64_t ldx, int64_t N, int D, const int64_t* edge_index, int64_t E,
    const uint8_t* code, const int32_t* src_rowptr, const int32_t* src_perm,
    const int32_t* tgt_rowptr, const int32_t* tgt_perm, double temperature, double gamma,
    double weight, double epsilon, const float* gout, const double* den, float* gx, int64_t ldg,
    spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(D <= PL_MAXD, "rows wider than 128 features are not supported");
  SPT_CHECK_ARG(pl_sizes_ok(N, E, D), "1 <= N, E < 2^31 and 1 <= D <= 128");
  SPT_CHECK_ARG(ldx >= D && ldg >= D, "row stride shorter than the row");
  SPT_CHECK_ARG(pl_params_ok(temperature, gamma, weight, epsilon),
                "temperature > 0, gamma >= 0, weight in [0, 1], epsilon in [0, 0.5)");
  SPT_CHECK_ARG(x && edge_index && code && src_rowptr && src_perm && tgt_rowptr && tgt_perm && gout &&
                    den && gx, "null pointer");
  SPT_CHECK_ARG(aligned_to(x, 4) && aligned_to(gx, 4) && aligned_to(edge_index, 8), "misaligned pointer");
  const FocalParams f = {1.0 / temperature, gamma, weight, epsilon};
  const bool vec = pl_vec(x, ldx, D), vec_out = pl_vec(gx, ldg, D);
  const int nblocks = (int)ceil_div(N, (int64_t)PL_GROUPS);
#define PL_BWD(NCH)                                                                              \
  pl_bwd_kernel<NCH><<<nblocks, PL_BLOCK, 0, stream>>>(x, ldx, N, D, vec, edge_index, E, code,    \
                                                       src_rowptr, src_perm, tgt_rowptr, tgt_perm, \
                                                       f, gout, den, gx, ldg, vec_out)
  switch ((D + 31) / 32) {
    case 1: PL_BWD(1); break;
    case 2: PL_BWD(2); break;
    case 3: PL_BWD(3); break;
    default: PL_BWD(4); break;
  }
#undef PL_BWD
  SPT_CHECK_LAUNCH();
  return 0;
}
