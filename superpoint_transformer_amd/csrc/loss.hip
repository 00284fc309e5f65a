// Cross-entropy of the classifier heads' logits (the criterion of the train step:
// configs/model/semantic/default.yaml:47-49 torch.nn.CrossEntropyLoss(ignore_index=num_classes),
// applied per output level in src/models/semantic.py; mean over the rows that are not ignored).
//
// [rows, C] logits with C = 13..32 classes: one lane per row keeps the row in registers, so
// log-sum-exp, the picked logit and (in the backward) the softmax cost one pass; the library's
// nll_loss forward / backward reduce with a single workgroup (0.26-0.42 ms per call at 428 571
// rows, profiles/r02z).  Sums are accumulated in f64 per workgroup and added up in a fixed order
// by a second kernel: deterministic.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "common.hpp"

namespace spt {

constexpr int CE_MAXC = 32;
constexpr int CE_BLOCK = 256;

template <int CMAX>
__global__ __launch_bounds__(CE_BLOCK) void ce_fwd_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ target, int64_t rows, int C,
    int64_t ignore_index, float* __restrict__ lse, double* __restrict__ partial) {
  __shared__ double s_sum[CE_BLOCK / 64], s_cnt[CE_BLOCK / 64];
  const int64_t row = (int64_t)blockIdx.x * CE_BLOCK + threadIdx.x;
  double li = 0.0, ci = 0.0;
  if (row < rows) {
    float v[CMAX];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      v[c] = (c < C) ? logits[row * C + c] : -INFINITY;
      m = fmaxf(m, v[c]);
    }
    float z = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) z += (c < C) ? expf(v[c] - m) : 0.f;
    const float lz = logf(z);
    lse[row] = m + lz;
    const int64_t t = target[row];
    if (t != ignore_index && t >= 0 && t < C) {
      float picked = 0.f;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) picked = (c == (int)t) ? v[c] : picked;
      // log z + (m - picked) in f64, as hl_fwd_kernel: the f32 sum m + log z carries ulp(|lse|),
      // which at logits near -3e4 is 2e-3 on a term of order 1
      li = (double)lz + ((double)m - (double)picked);
      ci = 1.0;
    } else if (t != ignore_index) {
      // a label outside [0, C) that is not ignore_index is a bug upstream (wrong num_classes,
      // unshifted void label): torch raises a device assert; here the loss comes out NaN instead
      // of silently averaging over fewer rows
      li = (double)NAN;
      ci = 1.0;
    }
  }
  // wave sums, then the block's four waves in order
  for (int o = 32; o > 0; o >>= 1) {
    li += __shfl_xor(li, o, 64);
    ci += __shfl_xor(ci, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = li;
    s_cnt[threadIdx.x >> 6] = ci;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < CE_BLOCK / 64; ++w) {
      a += s_sum[w];
      b += s_cnt[w];
    }
    partial[2 * (size_t)blockIdx.x] = a;
    partial[2 * (size_t)blockIdx.x + 1] = b;
  }
}

// loss = sum / max(count, 1) (0 when every row is ignored, like torch's nan-free convention is
// NOT: torch returns nan there; we return nan too by dividing 0 / 0 only when count == 0)
// (CountT: float for the plain CE, double for the weighted / histogram denominators)
template <typename CountT>
__global__ __launch_bounds__(256) void ce_finish_kernel(const double* __restrict__ partial, int nblocks,
                                                        float* __restrict__ loss,
                                                        CountT* __restrict__ count) {
  __shared__ double s_a[256], s_b[256];
  double a = 0.0, b = 0.0;
  const int per = (nblocks + 255) / 256;
  const int lo = threadIdx.x * per, hi = (lo + per < nblocks) ? lo + per : nblocks;
  for (int i = lo; i < hi; ++i) {
    a += partial[2 * (size_t)i];
    b += partial[2 * (size_t)i + 1];
  }
  s_a[threadIdx.x] = a;
  s_b[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    double ta = 0.0, tb = 0.0;
    for (int i = 0; i < 256; ++i) {
      ta += s_a[i];
      tb += s_b[i];
    }
    loss[0] = (float)(ta / tb);
    count[0] = (CountT)tb;
  }
}

template <int CMAX>
__global__ __launch_bounds__(CE_BLOCK) void ce_bwd_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ target, int64_t rows, int C,
    int64_t ignore_index, const float* __restrict__ gout, const float* __restrict__ count,
    float* __restrict__ glogits) {
  const int64_t row = (int64_t)blockIdx.x * CE_BLOCK + threadIdx.x;
  if (row >= rows) return;
  const int64_t t = target[row];
  const bool valid = t != ignore_index && t >= 0 && t < C;
  if (!valid) {                                // an explicit 0, whatever the row's logits hold
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) glogits[row * C + c] = 0.f;
    return;
  }
  // the softmax from the row's own max and sum, as hl_bwd_kernel (lse, an f32, is not read: its
  // rounding is ulp(|lse|) relative on every probability of the row)
  const double scale = (double)gout[0] / (double)count[0];
  float e[CMAX];
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    e[c] = (c < C) ? logits[row * C + c] : -INFINITY;
    m = fmaxf(m, e[c]);
  }
  float z = 0.f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    e[c] = (c < C) ? expf(e[c] - m) : 0.f;
    z += e[c];
  }
  const double rz = 1.0 / (double)z;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C)
      glogits[row * C + c] = (float)(((double)e[c] * rz - ((int)t == c ? 1.0 : 0.0)) * scale);
}

// ---- class-weighted CE on index targets, on the dominant label of a histogram, or against the
// whole histogram (the reference's default criterion: loss_type 'ce_kl', weighted_loss True) -----
//
// target: int64 [rows] labels (HL_INDEX) or int64 [rows, ncols] label counts with ncols in
// {C, C + 1}, column C = void (HL_DOMINANT, HL_HISTOGRAM).  Per row r, with l = logsumexp(z[r]):
//   index / dominant: num = w[t] (l - z[r, t]),                     den = w[t]
//   histogram:        num = sum_{c < C} h[r, c] w[c] (l - z[r, c]), den = sum_{c < ncols} h[r, c]
// loss = sum num / sum den.  The backward recomputes the row's softmax from the logits (max and
// sum, not a stored f32 log-sum-exp: rounding l to f32 alone costs 4.8e-7 relative on every
// probability of a row with |l| >= 8) and forms S_r p - h w in f64.
enum { HL_INDEX = 0, HL_DOMINANT = 1, HL_HISTOGRAM = 2 };

// the ncols <= CMAX + 1 counts of a histogram row into registers (0 beyond them); 16-byte loads
// when the base and the row stride (8 ncols bytes) keep every row 16-byte aligned
template <int CMAX>
__device__ __forceinline__ void load_hist_row(const int64_t* __restrict__ h, int64_t row, int ncols,
                                              int64_t (&hr)[CMAX + 2]) {
  const int64_t* p = h + row * ncols;
  if ((ncols & 1) == 0 && (reinterpret_cast<uintptr_t>(h) & 15) == 0) {
    const longlong2* p2 = reinterpret_cast<const longlong2*>(p);
#pragma unroll
    for (int k = 0; k < (CMAX + 2) / 2; ++k) {
      longlong2 q = make_longlong2(0, 0);
      if (2 * k < ncols) q = p2[k];          // 2k + 1 < ncols: ncols is even
      hr[2 * k] = q.x;
      hr[2 * k + 1] = q.y;
    }
  } else {
#pragma unroll
    for (int c = 0; c < CMAX + 2; ++c) hr[c] = (c < ncols) ? p[c] : 0;
  }
}

// the row's target class for HL_INDEX (a label) / HL_DOMINANT (hr = the row's counts): valid = the
// row counts, poison = a label that is neither a class nor ignored / a negative count
template <int CMAX>
__device__ __forceinline__ void row_label(int mode, const int64_t* __restrict__ target, int64_t row,
                                          const int64_t (&hr)[CMAX + 2], int C, int ncols,
                                          int64_t ignore_index, int& t, bool& valid, bool& poison) {
  if (mode == HL_INDEX) {
    const int64_t tt = target[row];
    valid = tt != ignore_index && tt >= 0 && tt < C;
    poison = !valid && tt != ignore_index;
    t = valid ? (int)tt : 0;
  } else {
    int64_t best = hr[0];
    t = 0;
    poison = hr[0] < 0;
#pragma unroll
    for (int c = 1; c < CMAX + 1; ++c) {
      if (c < ncols) {
        poison = poison || hr[c] < 0;
        if (hr[c] > best) {                  // strict: the first maximum wins (torch.argmax)
          best = hr[c];
          t = c;
        }
      }
    }
    valid = t < C;                           // a void-dominant row is ignored
  }
}

template <int CMAX>
__global__ __launch_bounds__(CE_BLOCK) void hl_fwd_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ target, int64_t rows, int C,
    int ncols, int mode, int64_t ignore_index, const float* __restrict__ weight,
    double* __restrict__ partial, int64_t* __restrict__ confmat) {
  __shared__ double s_sum[CE_BLOCK / 64], s_den[CE_BLOCK / 64];
  __shared__ float s_w[CE_MAXC];
  __shared__ unsigned long long s_cm[CE_MAXC * CE_MAXC];
  if (threadIdx.x < CE_MAXC) s_w[threadIdx.x] = (weight && (int)threadIdx.x < C) ? weight[threadIdx.x] : 1.f;
  if (confmat)
    for (int i = threadIdx.x; i < C * C; i += CE_BLOCK) s_cm[i] = 0ull;
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * CE_BLOCK + threadIdx.x;
  double num = 0.0, den = 0.0;
  if (row < rows) {
    float v[CMAX];
    float m = -INFINITY;
    int pred = 0;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      v[c] = (c < C) ? logits[row * C + c] : -INFINITY;
      if (v[c] > m) {                        // strict: the first maximum wins
        m = v[c];
        pred = c;
      }
    }
    float z = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) z += (c < C) ? expf(v[c] - m) : 0.f;
    const double l = (double)m + (double)logf(z);
    int64_t hr[CMAX + 2];
    if (mode != HL_INDEX) load_hist_row<CMAX>(target, row, ncols, hr);
    if (mode == HL_HISTOGRAM) {
      int64_t total = 0;
      bool poison = false;
#pragma unroll
      for (int c = 0; c < CMAX + 1; ++c) {
        total += hr[c];
        poison = poison || hr[c] < 0;
      }
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        // (a zero count meets v = -inf past C, or a masked logit: keep it out of the product)
        if (c < C && hr[c] != 0) num += (double)hr[c] * (double)s_w[c] * (l - (double)v[c]);
      }
      den = (double)total;
      if (poison) num = (double)NAN;
    } else {
      int t;
      bool valid, poison;
      row_label<CMAX>(mode, target, row, hr, C, ncols, ignore_index, t, valid, poison);
      if (valid) {
        float picked = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) picked = (c == t) ? v[c] : picked;
        den = (double)s_w[t];
        num = den * (l - (double)picked);
      }
      if (poison) {
        num = (double)NAN;
        den = 1.0;
      }
    }
    if (confmat && mode != HL_INDEX) {
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if (c < C && hr[c] != 0) atomicAdd(&s_cm[c * C + pred], (unsigned long long)hr[c]);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    num += __shfl_xor(num, o, 64);
    den += __shfl_xor(den, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = num;
    s_den[threadIdx.x >> 6] = den;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < CE_BLOCK / 64; ++w) {
      a += s_sum[w];
      b += s_den[w];
    }
    partial[2 * (size_t)blockIdx.x] = a;
    partial[2 * (size_t)blockIdx.x + 1] = b;
  }
  if (confmat)                               // integer sums: any arrival order gives the same table
    for (int i = threadIdx.x; i < C * C; i += CE_BLOCK)
      if (s_cm[i]) atomicAdd(reinterpret_cast<unsigned long long*>(confmat) + i, s_cm[i]);
}

template <int CMAX>
__global__ __launch_bounds__(CE_BLOCK) void hl_bwd_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ target, int64_t rows, int C,
    int ncols, int mode, int64_t ignore_index, const float* __restrict__ weight,
    const float* __restrict__ gout, const double* __restrict__ den, float* __restrict__ glogits) {
  __shared__ float s_w[CE_MAXC];
  if (threadIdx.x < CE_MAXC) s_w[threadIdx.x] = (weight && (int)threadIdx.x < C) ? weight[threadIdx.x] : 1.f;
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * CE_BLOCK + threadIdx.x;
  if (row >= rows) return;
  const double scale = (double)gout[0] / den[0];
  float e[CMAX];
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    e[c] = (c < C) ? logits[row * C + c] : -INFINITY;
    m = fmaxf(m, e[c]);
  }
  float z = 0.f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    e[c] = (c < C) ? expf(e[c] - m) : 0.f;
    z += e[c];
  }
  const double rz = 1.0 / (double)z;
  int64_t hr[CMAX + 2];
  if (mode != HL_INDEX) load_hist_row<CMAX>(target, row, ncols, hr);
  if (mode == HL_HISTOGRAM) {
    double S = 0.0;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) S += (c < C) ? (double)hr[c] * (double)s_w[c] : 0.0;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C)
        glogits[row * C + c] =
            (float)((S * ((double)e[c] * rz) - (double)hr[c] * (double)s_w[c]) * scale);
  } else {
    int t;
    bool valid, poison;
    row_label<CMAX>(mode, target, row, hr, C, ncols, ignore_index, t, valid, poison);
    const double S = valid ? (double)s_w[t] : 0.0;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) glogits[row * C + c] = (float)(S * ((double)e[c] * rz - (c == t ? 1.0 : 0.0)) * scale);
  }
}

// confmat[t, pred[r]] += h[r, t] for t < C (ncols >= C histogram columns; those past C are void),
// or, ncols == 0, confmat[target[r], pred[r]] += 1 for labels in [0, C).  Rows whose prediction
// is not a class are dropped.
__global__ __launch_bounds__(CE_BLOCK) void confusion_kernel(
    const int64_t* __restrict__ pred, const int64_t* __restrict__ target, int64_t rows, int C,
    int ncols, int64_t* __restrict__ confmat) {
  __shared__ unsigned long long s_cm[CE_MAXC * CE_MAXC];
  for (int i = threadIdx.x; i < C * C; i += CE_BLOCK) s_cm[i] = 0ull;
  __syncthreads();
  for (int64_t row = (int64_t)blockIdx.x * CE_BLOCK + threadIdx.x; row < rows;
       row += (int64_t)gridDim.x * CE_BLOCK) {
    const int64_t p = pred[row];
    if (p < 0 || p >= C) continue;
    if (ncols == 0) {
      const int64_t t = target[row];
      if (t >= 0 && t < C) atomicAdd(&s_cm[(int)t * C + (int)p], 1ull);
    } else {
      const int64_t* h = target + row * ncols;
      for (int c = 0; c < C; ++c) {
        const int64_t x = h[c];
        if (x != 0) atomicAdd(&s_cm[c * C + (int)p], (unsigned long long)x);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * C; i += CE_BLOCK)
    if (s_cm[i]) atomicAdd(reinterpret_cast<unsigned long long*>(confmat) + i, s_cm[i]);
}

// ---- edge-affinity loss of the panoptic model (src/models/panoptic.py:760-796) -------------------
//
// BCE with logits over the edges of obj_edge_index that do not join two void nodes, optionally
// weighted by the edge's case (same / different class x same / different object of the end nodes'
// major objects) and by pos_weight.  One pass: the keep mask, the case, the weight, the term and
// the tp / fp / tn / fn of `x > 0` against `t > 0.5` per edge; nothing is compacted.  The term is
// evaluated in f64 (exp, log1p), so the sum carries no error of an f32 transcendental; partial
// sums per workgroup in f64, added in a fixed order by ce_finish_kernel<double>: deterministic.
constexpr int EA_BLOCK = 256;

struct EdgeCase {
  bool keep;       // both ends in range and not both void
  bool bad;        // an end outside [0, N)
  int kind;        // 2 * (y_i != y_j) + (obj_i != obj_j)
};

__device__ __forceinline__ EdgeCase edge_case(const int64_t* __restrict__ ei, int64_t E, int64_t e,
                                              const uint8_t* __restrict__ node_void,
                                              const int64_t* __restrict__ node_obj,
                                              const int64_t* __restrict__ node_y, int64_t N) {
  EdgeCase c = {false, false, 0};
  const int64_t i = ei[e], j = ei[E + e];
  if (i < 0 || i >= N || j < 0 || j >= N) {    // compared with the bound before it indexes a table
    c.bad = true;
    return c;
  }
  c.keep = !(node_void[i] && node_void[j]);
  c.kind = 2 * (node_y[i] != node_y[j]) + (node_obj[i] != node_obj[j]);
  return c;
}

__global__ __launch_bounds__(EA_BLOCK) void ea_fwd_kernel(
    const float* __restrict__ logits, const float* __restrict__ target,
    const int64_t* __restrict__ ei, int64_t E, const uint8_t* __restrict__ node_void,
    const int64_t* __restrict__ node_obj, const int64_t* __restrict__ node_y, int64_t N,
    const float* __restrict__ case_weight, const float* __restrict__ pos_weight,
    double* __restrict__ partial, int64_t* __restrict__ stats, int32_t* __restrict__ status) {
  __shared__ double s_num[EA_BLOCK / 64], s_den[EA_BLOCK / 64];
  __shared__ int s_st[4][EA_BLOCK / 64];
  const int64_t e = (int64_t)blockIdx.x * EA_BLOCK + threadIdx.x;
  const double pw = pos_weight ? (double)pos_weight[0] : 1.0;
  double num = 0.0, den = 0.0;
  int what = -1;                               // 0 tp, 1 fp, 2 tn, 3 fn of a kept edge
  if (e < E) {
    const EdgeCase c = edge_case(ei, E, e, node_void, node_obj, node_y, N);
    if (c.bad && status) atomicAdd(&status[0], 1);
    if (c.keep) {
      const float xf = logits[e], tf = target[e];
      const double x = (double)xf, t = (double)tf;
      const double w = case_weight ? (double)case_weight[c.kind] : 1.0;
      // torch's stable form of BCE with logits
      const double l = (1.0 - t) * x +
                       (1.0 + (pw - 1.0) * t) * (fmax(-x, 0.0) + log1p(exp(-fabs(x))));
      num = w * l;
      den = w;
      what = (xf > 0.f) ? (tf > 0.5f ? 0 : 1) : (tf > 0.5f ? 3 : 2);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    num += __shfl_xor(num, o, 64);
    den += __shfl_xor(den, o, 64);
  }
  const int wave = threadIdx.x >> 6;
  if (stats) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int n = __popcll(__ballot(what == k));
      if ((threadIdx.x & 63) == 0) s_st[k][wave] = n;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    s_num[wave] = num;
    s_den[wave] = den;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < EA_BLOCK / 64; ++w) {
      a += s_num[w];
      b += s_den[w];
    }
    partial[2 * (size_t)blockIdx.x] = a;
    partial[2 * (size_t)blockIdx.x + 1] = b;
  }
  if (stats && threadIdx.x < 4) {              // integer sums: any arrival order gives the same
    int n = 0;
    for (int w = 0; w < EA_BLOCK / 64; ++w) n += s_st[threadIdx.x][w];
    if (n) atomicAdd(reinterpret_cast<unsigned long long*>(stats) + threadIdx.x, (unsigned long long)n);
  }
}

__global__ __launch_bounds__(EA_BLOCK) void ea_bwd_kernel(
    const float* __restrict__ logits, const float* __restrict__ target,
    const int64_t* __restrict__ ei, int64_t E, const uint8_t* __restrict__ node_void,
    const int64_t* __restrict__ node_obj, const int64_t* __restrict__ node_y, int64_t N,
    const float* __restrict__ case_weight, const float* __restrict__ pos_weight,
    const float* __restrict__ gout, const double* __restrict__ den, float* __restrict__ glogits) {
  const int64_t e = (int64_t)blockIdx.x * EA_BLOCK + threadIdx.x;
  if (e >= E) return;
  const EdgeCase c = edge_case(ei, E, e, node_void, node_obj, node_y, N);
  float g = 0.f;                               // a dropped edge: an explicit 0, never 0 * (1 / den)
  if (c.keep) {
    const double pw = pos_weight ? (double)pos_weight[0] : 1.0;
    const double x = (double)logits[e], t = (double)target[e];
    const double w = case_weight ? (double)case_weight[c.kind] : 1.0;
    // (1 - t) - (1 + (pw - 1) t) sigmoid(-x) in the form torch's own backward evaluates,
    // (1 + (pw - 1) t) sigmoid(x) - pw t: nothing cancels where sigmoid(x) vanishes
    const double sig = 1.0 / (1.0 + exp(-x));  // exp(-x) = inf gives 0
    g = (float)((double)gout[0] * w / den[0] * ((1.0 + (pw - 1.0) * t) * sig - pw * t));
  }
  glogits[e] = g;
}

}  // namespace spt

using namespace spt;

extern "C" size_t spt_edge_affinity_loss_workspace_bytes(int64_t E) {
  if (E < 1 || E >= (int64_t)INT32_MAX * EA_BLOCK) return 0;
  return (size_t)ceil_div(E, (int64_t)EA_BLOCK) * 2 * sizeof(double);
}

static bool ea_sizes_ok(int64_t E, int64_t N) {
  return E >= 1 && E < (int64_t)INT32_MAX * EA_BLOCK && N >= 1;
}

// loss[0] = sum w l / sum w over the kept edges (w = case_weight[case], or 1 without a table: the
// mean), den[0] = sum w as f64; no kept edge: 0 / 0 = NaN.  stats (optional) int64 [4] += tp, fp,
// tn, fn of (logit > 0) against (target > 0.5) over the kept edges; status (optional) int32 [1] +=
// edges with an end outside [0, N), which are dropped.
extern "C" int spt_edge_affinity_loss_fwd_f32(
    const float* logits, const float* target, const int64_t* edge_index, int64_t E,
    const uint8_t* node_void, const int64_t* node_obj, const int64_t* node_y, int64_t N,
    const float* case_weight, const float* pos_weight, float* loss, double* den, int64_t* stats,
    int32_t* status, void* ws, size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(ea_sizes_ok(E, N), "E >= 1 and N >= 1");
  SPT_CHECK_ARG(logits && target && edge_index && node_void && node_obj && node_y && loss && den,
                "null pointer");
  SPT_CHECK_ARG(ws && ws_bytes >= spt_edge_affinity_loss_workspace_bytes(E), "workspace too small");
  const int nblocks = (int)ceil_div(E, (int64_t)EA_BLOCK);
  double* partial = (double*)ws;
  ea_fwd_kernel<<<nblocks, EA_BLOCK, 0, stream>>>(logits, target, edge_index, E, node_void,
                                                  node_obj, node_y, N, case_weight, pos_weight,
                                                  partial, stats, status);
  ce_finish_kernel<double><<<1, 256, 0, stream>>>(partial, nblocks, loss, den);
  SPT_CHECK_LAUNCH();
  return 0;
}

// glogits[e] = gout[0] w / den[0] ((1 + (pw - 1) t) sigmoid(x) - pw t) for a kept edge, 0 for
// a dropped one (also when den is 0 or NaN).  gout, den, pos_weight are DEVICE scalars.
extern "C" int spt_edge_affinity_loss_bwd_f32(
    const float* logits, const float* target, const int64_t* edge_index, int64_t E,
    const uint8_t* node_void, const int64_t* node_obj, const int64_t* node_y, int64_t N,
    const float* case_weight, const float* pos_weight, const float* gout, const double* den,
    float* glogits, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(ea_sizes_ok(E, N), "E >= 1 and N >= 1");
  SPT_CHECK_ARG(logits && target && edge_index && node_void && node_obj && node_y && gout && den &&
                    glogits, "null pointer");
  const int nblocks = (int)ceil_div(E, (int64_t)EA_BLOCK);
  ea_bwd_kernel<<<nblocks, EA_BLOCK, 0, stream>>>(logits, target, edge_index, E, node_void,
                                                  node_obj, node_y, N, case_weight, pos_weight,
                                                  gout, den, glogits);
  SPT_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t spt_cross_entropy_workspace_bytes(int64_t rows) {
  return (size_t)(ceil_div(rows > 0 ? rows : 1, (int64_t)CE_BLOCK)) * 2 * sizeof(double);
}

// loss[0] = mean over the rows with target != ignore_index of (logsumexp(logits[row]) -
// logits[row, target[row]]); lse[rows] = the rows' f32 log-sum-exp (written as the entry promises;
// the backward takes it and does not read it); count[0] = number of such rows.
extern "C" int spt_cross_entropy_fwd_f32(const float* logits, const int64_t* target, int64_t rows,
                                         int C, int64_t ignore_index, float* lse, float* loss,
                                         float* count, void* ws, size_t ws_bytes,
                                         spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(rows >= 1 && C >= 1 && C <= CE_MAXC, "rows >= 1, 1 <= C <= 32");
  SPT_CHECK_ARG(logits && target && lse && loss && count, "null pointer");
  SPT_CHECK_ARG(ws && ws_bytes >= spt_cross_entropy_workspace_bytes(rows), "workspace too small");
  const int nblocks = (int)ceil_div(rows, (int64_t)CE_BLOCK);
  double* partial = (double*)ws;
  if (C <= 16)
    ce_fwd_kernel<16><<<nblocks, CE_BLOCK, 0, stream>>>(logits, target, rows, C, ignore_index, lse, partial);
  else
    ce_fwd_kernel<32><<<nblocks, CE_BLOCK, 0, stream>>>(logits, target, rows, C, ignore_index, lse, partial);
  ce_finish_kernel<float><<<1, 256, 0, stream>>>(partial, nblocks, loss, count);
  SPT_CHECK_LAUNCH();
  return 0;
}

// glogits[row, c] = (softmax(logits[row])[c] - [c == target[row]]) * gout[0] / count[0], 0 for
// ignored rows.  gout and count are DEVICE scalars (no host round trip).
extern "C" int spt_cross_entropy_bwd_f32(const float* logits, const int64_t* target,
                                         const float* lse, int64_t rows, int C,
                                         int64_t ignore_index, const float* gout,
                                         const float* count, float* glogits, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(rows >= 1 && C >= 1 && C <= CE_MAXC, "rows >= 1, 1 <= C <= 32");
  SPT_CHECK_ARG(logits && target && lse && gout && count && glogits, "null pointer");
  const int nblocks = (int)ceil_div(rows, (int64_t)CE_BLOCK);
  if (C <= 16)
    ce_bwd_kernel<16><<<nblocks, CE_BLOCK, 0, stream>>>(logits, target, rows, C, ignore_index, gout, count, glogits);
  else
    ce_bwd_kernel<32><<<nblocks, CE_BLOCK, 0, stream>>>(logits, target, rows, C, ignore_index, gout, count, glogits);
  SPT_CHECK_LAUNCH();
  return 0;
}

static bool hl_shape_ok(int mode, int C, int ncols) {
  if (mode == HL_INDEX) return true;
  return (mode == HL_DOMINANT || mode == HL_HISTOGRAM) && (ncols == C || ncols == C + 1);
}

// Class-weighted CE on index targets (mode 0), on the dominant label of a label histogram (1) or
// against the whole histogram (2): see the kernels.  loss[0] = sum num / sum den, den[0] = the
// denominator as f64 (sum of w[t], or the histogram's total count).  confmat (optional, modes 1
// and 2): int64 [C, C], confmat[t, argmax z[r]] += h[r, t], ADDED to what the buffer holds.
extern "C" int spt_hist_loss_fwd_f32(const float* logits, const int64_t* target, int64_t rows, int C,
                                     int ncols, int mode, int64_t ignore_index, const float* weight,
                                     float* loss, double* den, int64_t* confmat, void* ws,
                                     size_t ws_bytes, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(rows >= 1 && C >= 1 && C <= CE_MAXC, "rows >= 1, 1 <= C <= 32");
  SPT_CHECK_ARG(hl_shape_ok(mode, C, ncols),
                "mode 0 (index), or 1 / 2 (dominant / histogram) with ncols in {C, C + 1}");
  SPT_CHECK_ARG(logits && target && loss && den, "null pointer");
  SPT_CHECK_ARG(!confmat || mode != HL_INDEX, "the fused confusion matrix needs histogram targets");
  SPT_CHECK_ARG(ws && ws_bytes >= spt_cross_entropy_workspace_bytes(rows), "workspace too small");
  const int nblocks = (int)ceil_div(rows, (int64_t)CE_BLOCK);
  double* partial = (double*)ws;
  if (C <= 16)
    hl_fwd_kernel<16><<<nblocks, CE_BLOCK, 0, stream>>>(logits, target, rows, C, ncols, mode, ignore_index, weight, partial, confmat);
  else
    hl_fwd_kernel<32><<<nblocks, CE_BLOCK, 0, stream>>>(logits, target, rows, C, ncols, mode, ignore_index, weight, partial, confmat);
  ce_finish_kernel<double><<<1, 256, 0, stream>>>(partial, nblocks, loss, den);
  SPT_CHECK_LAUNCH();
  return 0;
}

// glogits[r, c] = gout[0] (S_r softmax(z[r])[c] - hw[r, c]) / den[0]: hw = h w and S_r = sum_c hw
// in mode 2; hw = w[t] onehot(t), S_r = w[t] in modes 0 / 1 (0 for rows that do not count).
extern "C" int spt_hist_loss_bwd_f32(const float* logits, const int64_t* target, int64_t rows, int C,
                                     int ncols, int mode, int64_t ignore_index, const float* weight,
                                     const float* gout, const double* den, float* glogits,
                                     spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(rows >= 1 && C >= 1 && C <= CE_MAXC, "rows >= 1, 1 <= C <= 32");
  SPT_CHECK_ARG(hl_shape_ok(mode, C, ncols),
                "mode 0 (index), or 1 / 2 (dominant / histogram) with ncols in {C, C + 1}");
  SPT_CHECK_ARG(logits && target && gout && den && glogits, "null pointer");
  const int nblocks = (int)ceil_div(rows, (int64_t)CE_BLOCK);
  if (C <= 16)
    hl_bwd_kernel<16><<<nblocks, CE_BLOCK, 0, stream>>>(logits, target, rows, C, ncols, mode, ignore_index, weight, gout, den, glogits);
  else
    hl_bwd_kernel<32><<<nblocks, CE_BLOCK, 0, stream>>>(logits, target, rows, C, ncols, mode, ignore_index, weight, gout, den, glogits);
  SPT_CHECK_LAUNCH();
  return 0;
}

// confmat[t, pred[r]] += h[r, t] (t < C <= 32; ncols >= C) or, ncols == 0, += 1 at
// [target[r], pred[r]] for labels in [0, C); int64 [C, C], ADDED to what the buffer holds.
extern "C" int spt_confusion_matrix_i64(const int64_t* pred, const int64_t* target, int64_t rows,
                                        int C, int ncols, int64_t* confmat, spt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPT_CHECK_ARG(rows >= 1 && C >= 1 && C <= CE_MAXC, "rows >= 1, 1 <= C <= 32");
  SPT_CHECK_ARG(ncols == 0 || ncols >= C, "ncols == 0 (labels) or ncols >= C (histogram)");
  SPT_CHECK_ARG(pred && target && confmat, "null pointer");
  // few, long-lived workgroups: each flushes up to C * C cells with global atomics
  const int nblocks = (int)std::min<int64_t>(ceil_div(rows, (int64_t)CE_BLOCK), 1024);
  confusion_kernel<<<nblocks, CE_BLOCK, 0, stream>>>(pred, target, rows, C, ncols, confmat);
  SPT_CHECK_LAUNCH();
  return 0;
}
