/*
 * spt_hip.h — flat C ABI of libspt_hip.so, the MI355X (gfx950) hot path of
 * Superpoint Transformer.
 *
 * Every entry point replaces one call the reference makes into an un-vendored
 * native dependency (torch_scatter / torch_geometric / FRNN / pgeof) or one
 * multi-launch Python composite of those calls.  Reference citations are
 * file:line relative to drprojects/superpoint_transformer v3.0.0.
 *
 * Conventions
 *   - all pointers are DEVICE pointers owned by the caller (PyTorch's caching
 *     allocator in practice); the library never allocates device memory.
 *     Scratch comes from a caller-provided workspace (ws, ws_bytes) whose size
 *     is returned by the paired *_workspace_bytes() query;
 *   - every function is asynchronous on `stream` (a hipStream_t passed as
 *     void*) and re-entrant.  State held by the library: the thread-local
 *     last-error string, and a handful of process-wide FORMULATION DEFAULTS
 *     (std::atomic<int>, set by the spt_*_use_* / spt_attn_bwd_* setters below or
 *     read once from SPT_* environment variables: matrix-pipe precision, backward
 *     tiling, edge order, LDS-DMA staging, streaming segment-max, cell-centric
 *     kNN).  They select between implementations of the SAME result and apply
 *     only where a call passes no choice of its own: every op they govern has a
 *     *_ex / *_m entry whose `mode` word carries the choice per call, so two
 *     callers (threads, streams, models) never change each other's arithmetic;
 *   - return value: 0 = ok, <0 = error (see spt_last_error()).  Nothing throws
 *     across the boundary;
 *   - row-major, contiguous tensors; f32 features; int64 indices as the
 *     reference hands them over (NAGCast, src/transforms/data.py:54-150);
 *     int32 perm/rowptr inside CSR views (N0 < 2^31 rows);
 *   - base alignment: the kernels index rows from the base pointer and pick their vector width
 *     from the row length alone, so a [rows, c] f32 tensor (input, gradient or output) whose rows
 *     are whole 16-byte chunks (c % 4 == 0) must start on a 16-byte boundary (c % 2 == 0: 8 bytes;
 *     else its elements' 4), and so must the int32 arg rows written next to it; int64 index
 *     tensors are read one element at a time (8 bytes).  The segment (spt_segcsr_*,
 *     spt_gather_rows_f32), GraphNorm (spt_graphnorm_fwd / stats / bwd / bwd_acc / apply /
 *     bwd_stats), edge-affinity feature, unit-sphere assemble, attention (spt_edge_attn_*_ex_f32,
 *     spt_attn_split_*: also the encoders' weights Wk / Wq / Wv), tall-skinny Linear (x, W, Wt, gy) and fused-layer entries (x, W, h, gy,
 *     xprev, gx; the pool-fused pair also out, arg, argpos, raw; the fold's x0, W0, gW0) REFUSE a misaligned pointer with
 *     the other argument checks, before anything is launched (status < 0, the argument named in
 *     spt_last_error(), no output touched).  Memory from hipMalloc is 256-byte aligned; a view
 *     into the middle of an allocation need not be (the Python wrappers copy such a view);
 *   - segment ops take a CSR view (perm, rowptr) of an UNSORTED index built by
 *     spt_csr_build(): rows of segment s are perm[rowptr[s] .. rowptr[s+1]) in
 *     ascending original order (stable), so reductions are deterministic and
 *     the arg-tie rule is "first occurrence" like torch_scatter's CPU kernel.
 */
#ifndef SPT_HIP_H
#define SPT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* spt_stream_t; /* hipStream_t */

enum spt_reduce_op {
  SPT_SUM = 0,
  SPT_MEAN = 1,
  SPT_MIN = 2,
  SPT_MAX = 3
};

/* Round 6: a GraphNorm whose tables a fused layer call writes from the statistics it has just
 * summed, instead of the caller making a second call for them (spt_graphnorm_tables_f32 /
 * spt_graphnorm_bwd_tables_f32: same formulas, same bits).  HOST structs of DEVICE pointers, passed
 * by address and copied into the launch: weight / mean_scale [d] are the norm's parameters
 * (PyG GraphNorm, src/nn/mlp.py:85-94); the forward tables mean / rstd / am / scale are
 * [num_graphs, d]; the backward tables c1 / c2 / c3 [num_graphs, d] and the parameter gradients
 * gweight / gbias / gmean_scale [d]. */
typedef struct spt_gn_fwd_tables {
  const float* weight;
  const float* mean_scale;
  float eps;
  float* mean;
  float* rstd;
  float* am;
  float* scale;
} spt_gn_fwd_tables;
typedef struct spt_gn_bwd_tables {
  const float* weight;
  const float* mean_scale;
  const float* mean;
  const float* rstd;
  float* c1;
  float* c2;
  float* c3;
  float* gweight;
  float* gbias;
  float* gmean_scale;
} spt_gn_bwd_tables;

/* Library ABI version (major*1000 + minor). */
int spt_version(void);
/* Thread-local description of the last error returned by this library. */
const char* spt_last_error(void);

/* ------------------------------------------------------------------------
 * CSR view of an unsorted segment index.
 * Replaces the implicit "group by index" that every torch_scatter COO kernel
 * redoes with atomics (call sites: src/nn/pool.py:61-62, src/nn/norm.py:118-126,
 * src/nn/attention.py:307,315, src/data/nag.py:97,108).
 *   idx     [n]          int64, values in [0, num_seg)
 *   perm    [n]          int32 out: stable argsort of idx
 *   rowptr  [num_seg+1]  int32 out: segment s owns perm[rowptr[s]..rowptr[s+1])
 * ---------------------------------------------------------------------- */
size_t spt_csr_build_workspace_bytes(int64_t n, int64_t num_seg);
int spt_csr_build(const int64_t* idx, int64_t n, int64_t num_seg,
                  int32_t* perm, int32_t* rowptr,
                  void* ws, size_t ws_bytes, spt_stream_t stream);
/* Companions of the view: pos_seg[j] = segment of CSR position j (= idx[perm[j]], expanded from
 * rowptr: no gather), and out[j] = (int32) src[perm[j]] (e.g. edge_index[1] in CSR order) - one
 * kernel each where the host side used three torch launches (cast, index_select, cast). */
int spt_csr_pos_seg(const int32_t* rowptr, int64_t num_seg, int64_t n, int32_t* pos_seg,
                    spt_stream_t stream);
int spt_csr_gather_i64_i32(const int64_t* src, const int32_t* perm, int64_t n, int32_t* out,
                           spt_stream_t stream);
/* The by-source view of an attention graph and every table a level's attention calls derive from
 * it, in one entry (11 launches for the three sort passes of 17 .. 24 key bits; the entries above
 * and spt_attn_mirror_prepare / spt_attn_pack_tile_ids_mirror took about 22 for the same arrays,
 * bit for bit).
 * `edge_index` = the [2, e] int64 list (e >= 1), n = the number of nodes, `pairs` = M of a list
 * declared [i<j | j>i | loops] (see spt_attn_mirror_prepare) or -1.  Written, all int32:
 * erowptr [n + 1], eperm [e] (the stable order by source), tgt_sorted [e] = edge_index[1][eperm],
 * src_sorted [e] = edge_index[0][eperm], inv [e] = the inverse of eperm (NULL: not wanted),
 * tile_ids [ceil(e / 16), 64] = the records of spt_attn_pack_tile_ids_mirror (NULL: not wanted;
 * needs pairs >= 0 and inv), *flag = the verdict of the mirror check (same bits; 0 for
 * pairs = -1) - WRITTEN, not OR-ed: the caller does not clear it. */
size_t spt_edge_csr_build_workspace_bytes(int64_t e, int64_t n);
int spt_edge_csr_build(const int64_t* edge_index, int64_t e, int64_t n, int64_t pairs,
                       int32_t* erowptr, int32_t* eperm, int32_t* tgt_sorted, int32_t* src_sorted,
                       int32_t* inv, int32_t* tile_ids, int32_t* flag, void* ws, size_t ws_bytes,
                       spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Segment reduce  out[s,:] = reduce_{i in seg s} x[i,:]      (a1, a4, a8)
 * Replaces torch_scatter.scatter / scatter_{sum,mean,min,max} and the PyG
 * {Sum,Mean,Min,Max}Aggregation the pools dispatch to
 * (src/nn/pool.py:61-82 <- src/nn/stage.py:429-431; src/nn/norm.py:118-126).
 *   x    [n,c] f32      out [num_seg,c] f32
 *   arg  [num_seg,c] int32 or NULL: for MIN/MAX the row index of the selected
 *        element, n for an empty segment (torch_scatter's sentinel).
 * Empty segments reduce to 0.  MEAN divides by max(count,1).
 * ---------------------------------------------------------------------- */
int spt_segcsr_reduce_f32(int op, const float* x, const int32_t* perm,
                          const int32_t* rowptr, int64_t n, int64_t num_seg,
                          int c, float* out, int32_t* arg, spt_stream_t stream);
/* Max + arg of 128-channel rows over >= 65 536 rows (the level-0 -> level-1 pool) runs a
 * row-streaming kernel: a wave owns a contiguous range of CSR positions cut at segment boundaries
 * and streams sixteen 512-byte rows at a time whatever segments they belong to (1, default;
 * SPT_SEG_STREAM=0 in the environment or 0 here = the lane-group-per-segment kernel for every
 * shape).  Bit-identical results.  Returns the previous setting. */
int spt_segcsr_use_stream(int on);
/* Same two entries with the formulation chosen PER CALL (-1: process default, 0: lane group per
 * segment, 1: row-streaming where it applies); they touch no process-wide state. */
int spt_segcsr_reduce_ex_f32(int op, const float* x, const int32_t* perm,
                             const int32_t* rowptr, int64_t n, int64_t num_seg,
                             int c, float* out, int32_t* arg, int formulation,
                             spt_stream_t stream);
int spt_segcsr_max_affine_ex_f32(const float* x, const int32_t* perm, const int32_t* rowptr,
                                 int64_t n, int64_t num_seg, int c, const float* am,
                                 const float* scale, const float* bias, float act_slope,
                                 const int64_t* seg_graph, float* out, int32_t* arg,
                                 int formulation, spt_stream_t stream);

/* Backward of the above w.r.t. x (a2):
 *   SUM : gx[i,:] = gout[idx[i],:]
 *   MEAN: gx[i,:] = gout[idx[i],:] / max(count[idx[i]],1)
 *   MIN/MAX: gx[i,c] = gout[idx[i],c] if arg[idx[i],c]==i else 0
 * (torch_scatter routes the gradient to the single arg element.)           */
/* Max-pool of y = leaky(scale[g] (x - am[g]) + bias) computed on the fly from the RAW x:
 * the GraphNorm-apply + LeakyReLU that ends the point MLP (src/nn/mlp.py:46-50) folded into
 * the L0 -> L1 pool read (src/nn/pool.py:61-82).  am / scale [B, c] per graph, bias [c],
 * seg_graph [num_seg] int64 graph of each segment (NULL = one graph); out / arg as above.
 * Same values and arg as applying the norm first, without writing the normalised rows. */
int spt_segcsr_max_affine_f32(const float* x, const int32_t* perm, const int32_t* rowptr,
                              int64_t n, int64_t num_seg, int c, const float* am,
                              const float* scale, const float* bias, float act_slope,
                              const int64_t* seg_graph, float* out, int32_t* arg,
                              spt_stream_t stream);
/* Same with x stored as bf16 [n, c] (SPT_FMLP_H_BF16 below); built for c = 128, n >= 65 536. */
int spt_segcsr_max_affine_bf16_supported(int c, int64_t n);
int spt_segcsr_max_affine_bf16(const void* x_bf16, const int32_t* perm, const int32_t* rowptr,
                               int64_t n, int64_t num_seg, int c, const float* am,
                               const float* scale, const float* bias, float act_slope,
                               const int64_t* seg_graph, float* out, int32_t* arg,
                               spt_stream_t stream);
/* Same pool (x f32, or bf16 rows with x_is_bf16 != 0) with a third output raw [num_seg, c] f32 =
 * x[arg[s, c], c], the winner's value BEFORE the map (0 for an empty segment): what the top
 * GraphNorm's backward statistics of a max-pooled layer need (spt_graphnorm_bwd_stats_sparse_raw_f32
 * reads it as a stream instead of gathering).  Built for c = 128, n >= 65 536. */
int spt_segcsr_max_affine_raw_supported(int c, int64_t n);
int spt_segcsr_max_affine_raw_f32(const void* x, int x_is_bf16, const int32_t* perm,
                                  const int32_t* rowptr, int64_t n, int64_t num_seg, int c,
                                  const float* am, const float* scale, const float* bias,
                                  float act_slope, const int64_t* seg_graph, float* out,
                                  int32_t* arg, float* raw, spt_stream_t stream);
int spt_segcsr_reduce_bwd_f32(int op, const float* gout, const int32_t* arg,
                              const int64_t* idx, const int32_t* perm,
                              const int32_t* rowptr, int64_t n, int64_t num_seg,
                              int c, float* gx, spt_stream_t stream);

/* Wide rows (>= 128 B) stream in CSR order when perm/rowptr are given (the
 * parent row is read once per segment); narrow rows run in idx order. */

/* Bit-exact integer segment sum (a8: NAG.get_sub_size, src/data/nag.py:59-110). */
int spt_segcsr_sum_i64(const int64_t* x, const int32_t* perm,
                       const int32_t* rowptr, int64_t n, int64_t num_seg,
                       int c, int64_t* out, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Row gather  out[i,:] = x[idx[i],:]                               (a3)
 * Replaces IndexUnpool (src/nn/unpool.py:12-13) and the parent->child
 * broadcasts of src/nn/norm.py:132-133, src/nn/stage.py:269.  Its backward
 * is spt_segcsr_reduce_f32(SPT_SUM) on the CSR view of idx.
 * ---------------------------------------------------------------------- */
int spt_gather_rows_f32(const float* x, const int64_t* idx, int64_t n,
                        int64_t num_src, int c, float* out, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused UnitSphereNorm                                              (a4)
 * Replaces UnitSphereNorm._forward_scatter / _forward
 * (src/nn/norm.py:86-138 <- src/nn/stage.py:250) and its helper
 * scatter_mean_weighted (src/utils/scatter.py:17-38): per segment bounding
 * box -> diameter = max axis span; centre = (weighted) mean;
 * pos_out = (pos - centre[idx]) / (diameter[idx] + 1e-2).
 *   pos [n,3] f32; idx [n] int64 (NULL = one segment, norm.py:86-110);
 *   (perm, rowptr) = CSR view of idx; w_f32 / w_i64: optional weights (at
 *   most one non-NULL; int64 node_size is cast to f32 like the reference);
 *   pos_out [n,3], diam [num_seg], center [num_seg,3] f32 out.
 * Empty segment -> diameter 0, centre 0.  No gradient (positions are data).
 * ---------------------------------------------------------------------- */
int spt_unit_sphere_norm_f32(const float* pos, const int64_t* idx,
                             const int32_t* perm, const int32_t* rowptr,
                             const float* w_f32, const int64_t* w_i64,
                             int64_t n, int64_t num_seg, float* pos_out,
                             float* diam, float* center, spt_stream_t stream);
/* The same statistics with the stage's input assembly (src/nn/stage.py:249-271, the three
 * fusion concatenations for use_pos / use_diameter_parent) done by the writing pass:
 * xcat [n, 4 + cx] = [diam[idx] | pos_normalised | x], x [n, cx] with cx % 4 == 0 - the
 * normalised positions, the gathered parent diameter and the copy of x are never materialised. */
int spt_unit_sphere_assemble_f32(const float* pos, const int64_t* idx,
                                 const int32_t* perm, const int32_t* rowptr,
                                 const float* w_f32, const int64_t* w_i64,
                                 int64_t n, int64_t num_seg, const float* x, int cx,
                                 float* xcat, float* diam, float* center, spt_stream_t stream);
/* Both entries with a caller workspace of spt_unit_sphere_workspace_bytes(n, num_seg) bytes:
 * segments of thousands of rows (idx = NULL: the whole top level is one segment, norm.py:86-110)
 * are reduced by several workgroups each and merged in a fixed order instead of by one. */
size_t spt_unit_sphere_workspace_bytes(int64_t n, int64_t num_seg);
int spt_unit_sphere_norm_ws_f32(const float* pos, const int64_t* idx, const int32_t* perm,
                                const int32_t* rowptr, const float* w_f32, const int64_t* w_i64,
                                int64_t n, int64_t num_seg, float* pos_out, float* diam,
                                float* center, void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_unit_sphere_assemble_ws_f32(const float* pos, const int64_t* idx, const int32_t* perm,
                                    const int32_t* rowptr, const float* w_f32, const int64_t* w_i64,
                                    int64_t n, int64_t num_seg, const float* x, int cx, float* xcat,
                                    float* diam, float* center, void* ws, size_t ws_bytes,
                                    spt_stream_t stream);

/* ------------------------------------------------------------------------
 * GraphNorm forward / backward, optionally fused with LeakyReLU      (a5)
 * Replaces torch_geometric.nn.norm.GraphNorm (PyG 2.3.0, install.sh:100) as
 * called from src/nn/mlp.py:85-94 (every MLP layer, followed by the
 * LeakyReLU of mlp.py:46-50) and src/nn/transformer.py:258-265:
 *   mu = mean_g x; o = x - mean_scale*mu[batch]; var = mean_g o^2;
 *   y = weight * o / sqrt(var + eps) + bias;  y = leaky_relu(y, act_slope)
 *   x [r,d] f32; batch [r] int64 in [0,num_graphs) or NULL (one graph);
 *   act_slope = 1 disables the activation; mean, rstd [num_graphs,d] out
 *   (saved for the backward).  Statistics accumulate in f64 with a
 *   fixed-order reduction: results are run-to-run deterministic.
 * ws: caller workspace of spt_graphnorm_workspace_bytes(r,d,num_graphs).
 * ---------------------------------------------------------------------- */
size_t spt_graphnorm_workspace_bytes(int64_t r, int d, int num_graphs);
int spt_graphnorm_fwd_f32(const float* x, const int64_t* batch, int64_t r, int d,
                          int num_graphs, const float* weight, const float* bias,
                          const float* mean_scale, float eps, float act_slope,
                          float* y, float* mean, float* rstd, void* ws,
                          size_t ws_bytes, spt_stream_t stream);
int spt_graphnorm_bwd_f32(const float* x, const float* gy, const int64_t* batch,
                          int64_t r, int d, int num_graphs, const float* weight,
                          const float* bias, const float* mean_scale,
                          const float* mean, const float* rstd, float act_slope,
                          float* gx, float* gweight, float* gbias,
                          float* gmean_scale, void* ws, size_t ws_bytes,
                          spt_stream_t stream);
/* Statistics + coefficient tables only (no apply pass): mean, rstd and the rows of
 * y = (x - am[g]) * scale[g] + bias, all [num_graphs, d], for consumers that normalise on the fly
 * (spt_skinny_linear_pre_f32).  ws: spt_graphnorm_workspace_bytes(). */
int spt_graphnorm_stats_f32(const float* x, const int64_t* batch, int64_t r, int d, int num_graphs,
                            const float* weight, const float* mean_scale, float eps, float* mean,
                            float* rstd, float* am, float* scale, void* ws, size_t ws_bytes,
                            spt_stream_t stream);
/* spt_graphnorm_bwd_f32 with gx = gx_add + (backward of the norm); gx_add [r, d] or NULL: the
 * gradient of the residual branch around a pre-norm joins in the apply pass. */
int spt_graphnorm_bwd_acc_f32(const float* x, const float* gy, const int64_t* batch,
                              int64_t r, int d, int num_graphs, const float* weight,
                              const float* bias, const float* mean_scale,
                              const float* mean, const float* rstd, float act_slope,
                              const float* gx_add, float* gx, float* gweight, float* gbias,
                              float* gmean_scale, void* ws, size_t ws_bytes,
                              spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused sparse graph self-attention with relative-pose encodings   (a6.2-a6.7)
 * Replaces the body of SelfAttentionBlock.forward between the qkv and the
 * out_proj Linear (src/nn/attention.py:202-315): edge gathers q[s], k[t], v[t],
 * qk scaling (src/utils/nn.py:75-127), the k/q/v RPE Linears on edge_attr,
 * the per-head dot product, torch_geometric.utils.softmax over the edges of
 * each source node and the scatter_sum of the weighted values.
 *   qkv        [n, 2*H*D + H*Dv] f32: output of the block's own qkv Linear,
 *              columns [q | k | v], each head-major (attention.py:202-204)
 *   erowptr    [n+1], eperm [e] (NULL = edges already grouped by source):
 *              CSR view of edge_index[0] from spt_csr_build
 *   tgt_sorted [e] int32: edge_index[1] in CSR order (tgt[eperm[j]])
 *   edge_attr  [e, F] f32 in ORIGINAL edge order, or NULL (no RPE)
 *   Wk,bk / Wq,bq / Wv,bv: k_rpe / q_rpe / v_rpe Linear parameters
 *              ([H*D,F],[H*D],[H*Dv,F],[H*Dv]); any may be NULL (encoder absent)
 *   scale_mode/scale_a: 0: a*deg^-0.5 ('d.g', 'g'), 1: a + deg^-0.5 ('d+g'),
 *              2: a ('d' or a constant); deg(s) = erowptr[s+1]-erowptr[s]
 *   out [n, H*Dv]; m, z [n, H]: running max / sum of the softmax, saved for
 *              the backward (both NULL to skip).
 * Built shapes: H*D <= 128, H*Dv <= 128, F in {18, 32}; anything else returns
 * an error.  Which kernel a built shape runs on is decided by the mode word and
 * the route table further down.  Forward is deterministic.
 * Backward: gout [n, H*Dv] -> gqkv [n, ld] (zero-filled here; k/v columns use
 * f32 atomics), gedge_attr [e, F], and the six RPE parameter gradients
 * (NULL to skip one).  ws: spt_edge_attn_bwd_workspace_bytes().
 * ---------------------------------------------------------------------- */
int spt_edge_attn_fwd_f32(const float* qkv, int64_t n, int H, int D, int Dv,
                          const int32_t* erowptr, const int32_t* eperm,
                          const int32_t* tgt_sorted, int64_t e,
                          const float* edge_attr, int F, const float* Wk,
                          const float* bk, const float* Wq, const float* bq,
                          const float* Wv, const float* bv, int scale_mode,
                          float scale_a, float* out, float* m, float* z,
                          spt_stream_t stream);
size_t spt_edge_attn_bwd_workspace_bytes(int H, int D, int Dv, int F);
/* Three formulations exist for the SPT-64 head layout (H=16, D=Dv=4, F=32):
 *   2 (default)  matrix pipe, split-bf16: every f32 product of the three RPE GEMMs (and of
 *                the two gradient GEMMs) is hi*hi + lo*hi + hi*lo of bf16 halves on the bf16
 *                MFMA (16x the f32 pipe's rate), f32 accumulate: the dropped lo*lo term and the
 *                halves' rounding leave ~2^-17 relative per product (17 of f32's 24 bits);
 *   1            matrix pipe, f32 in / f32 accumulate (bitwise an fmaf chain);
 *   0            generic lane-per-output VALU kernels (every other shape uses these).
 * spt_attn_use_mfma(mode) selects process-wide and returns the previous mode (mode < -1: query
 * only, nothing changes); tests cross-check all three at full scene size. */
int spt_attn_use_mfma(int mode);
/* Backward tiling of the bf16-pipe modes (2, 3): 2 (default) = the edge-lane kernel described
 * below where the route table allows it; 1 = 16-edge tiles over the edge
 * stream, at most two consecutive source nodes per pass, tiles 100 % full (dq by atomicAdd: a
 * node may be cut between two waves); 0 = one tile set per source node (62-69 % full at mean
 * degree 16).  Same results up to f32 summation order.  Returns the previous setting. */
int spt_attn_bwd_packed(int on);
/* Request shape of the edge-lane backward's k / v gathers and [dk | dv] stores: 1 (default) = whole
 * 128-byte lines per instruction, 0 = the 64-byte pieces of the MFMA layout.  Results are bit-identical;
 * process-wide measurement switch (< 0: query), returns the previous setting. */
int spt_attn_bwd_el_full_line(int on);
/* Edge order of the edge-lane backward: 1 (default) = the edge stream sorted by TARGET node
 * (csrc/edge_attn_to.hip: k / v of the target are L1 hits, dk / dv are reduced inside the tile, the
 * streamed per-edge quantity is dq - half the bytes of [dk | dv]), 0 = by source
 * (csrc/edge_attn_el.hip).  Process-wide (< 0: query), returns the previous setting.  The tile
 * records a caller builds once per batch and level differ between the two:
 * spt_attn_pack_tile_ids_ex writes the format of the current setting, spt_attn_tile_record_ints()
 * ints per 16-edge tile (64 / 48). */
int spt_attn_bwd_el_target_order(int on);
int spt_attn_tile_record_ints(void);
int spt_attn_pack_tile_ids_ex(const int32_t* eperm, const int32_t* tgt_sorted,
                              const int32_t* src_sorted, const int32_t* tperm, int64_t e,
                              int32_t* tile_ids, spt_stream_t stream);
/* The same two with the edge order taken from bits 6-7 of a per-call `mode` word (< 0 or 0 in
 * those bits: the process default) - the word later handed to spt_edge_attn_bwd_ex_f32.
 * ABI note (round 4 -> 5): spt_attn_pack_tile_ids (48-int records, declared further down) REFUSES
 * while the process default is the target order, because records of the wrong width would be read
 * as garbage; callers of the older pair (spt_attn_pack_tile_ids + spt_edge_attn_bwd_ex_f32) either
 * move to the _m entries or pin SPT_ATTN_BWD_SOURCE_ORDER in their mode word and call
 * spt_attn_pack_tile_ids_m with it. */
int spt_attn_tile_record_ints_m(int mode);
int spt_attn_pack_tile_ids_m(const int32_t* eperm, const int32_t* tgt_sorted,
                             const int32_t* src_sorted, const int32_t* tperm, int64_t e, int mode,
                             int32_t* tile_ids, spt_stream_t stream);
/* Round 6: TARGET-order tile records without a sorted target view, from the MIRROR structure of
 * the reference's final edge list [i<j | j>i | loops] (src/transforms/graph.py:1268, 1442-1446:
 * OnTheFlyHorizontalEdgeFeatures appends the flipped copy of the trimmed list, NAGAddSelfLoops the
 * loops; the shipped S3DIS / DALES / ScanNet configs skip SampleEdges - `sample_edge_n_min: -1`).
 * `edge_index` = the [2, e] int64 list, `pairs` = M: edge i < M is mirrored at i + M, every edge
 * from 2 M on is a self loop.  The edges INTO a node are the mirrors of the edges OUT OF it, which
 * the by-source view (eperm) holds as one run: no second radix sort per level.
 * spt_attn_mirror_prepare writes inv [e] (int32: the inverse of eperm) and ORs into *flag (int32,
 * device; the caller clears it) bit 0 = a pair (i, i + M) that is not (s, t) / (t, s), bit 1 = a
 * loop with s != t - the structure is CHECKED, not trusted.  spt_attn_pack_tile_ids_mirror writes
 * the 64-int records of spt_attn_pack_tile_ids_m's target order (same fields; the edges into a
 * node in by-source order of their mirrors instead of ascending source: the same sums).
 * spt_edge_attn_bwd_ex_f32 accepts them with tperm = trowptr = NULL. */
int spt_attn_mirror_prepare(const int64_t* edge_index, const int32_t* eperm, int64_t e, int64_t pairs,
                            int32_t* inv, int32_t* flag, spt_stream_t stream);
int spt_attn_pack_tile_ids_mirror(const int32_t* eperm, const int32_t* tgt_sorted,
                                  const int32_t* src_sorted, const int32_t* inv, int64_t e,
                                  int64_t pairs, int32_t* tile_ids, spt_stream_t stream);
/* Round 6: operand layout of the head-group decomposition that runs wider head layouts on the
 * built 16 x (qk 4, value 4) kernels (H = 16 G heads of value dim 4 J; SPT-128 of
 * configs/experiment/semantic/kitti360.yaml:22-27: G = 1, J = 2 - src/nn/attention.py:202-315 is
 * linear in the value dims, so the passes are exact).  qkv rows are [q 64 G | k 64 G | v H x 4 J].
 * spt_attn_split_pack_f32: qa [G J, n, 192] <- per pass p = g J + j the columns
 *   [q_g | k_g | v_g[:, 4 j .. 4 j + 3]] of every row (what one index gather + one transposing copy did);
 * spt_attn_split_grad_f32: gqkv [n, 128 G + 64 G J] <- the passes' gradients gqa [G J, n, 192], the
 *   q / k columns summed over the J slices of their head group in ascending j, the v columns copied
 *   (what a sum, three permuting copies and a cat did).  16-byte aligned pointers. */
int spt_attn_split_pack_f32(const float* qkv, int64_t n, int G, int J, float* qa, spt_stream_t stream);
int spt_attn_split_grad_f32(const float* gqa, int64_t n, int G, int J, float* gqkv, spt_stream_t stream);
int spt_edge_attn_bwd_f32(const float* qkv, int64_t n, int H, int D, int Dv,
                          const int32_t* erowptr, const int32_t* eperm,
                          const int32_t* tgt_sorted, int64_t e,
                          const float* edge_attr, int F, const float* Wk,
                          const float* bk, const float* Wq, const float* bq,
                          const float* Wv, const float* bv, int scale_mode,
                          float scale_a, const float* out, const float* m,
                          const float* z, const float* gout, float* gqkv,
                          float* gedge_attr, float* gWk, float* gbk, float* gWq,
                          float* gbq, float* gWv, float* gbv, void* ws,
                          size_t ws_bytes, spt_stream_t stream);
/* Same with gedge_attr_accumulate != 0: d edge_attr is ADDED (f32 hardware atomics) to what
 * gedge_attr already holds instead of stored.  The transformer blocks of a stage all read the same
 * edge_attr (src/nn/stage.py:137-141), so their backward passes share one gradient buffer instead
 * of leaving autograd to sum 3-4 [E,F] tensors. */
int spt_edge_attn_bwd_acc_f32(const float* qkv, int64_t n, int H, int D, int Dv,
                              const int32_t* erowptr, const int32_t* eperm,
                              const int32_t* tgt_sorted, int64_t e,
                              const float* edge_attr, int F, const float* Wk,
                              const float* bk, const float* Wq, const float* bq,
                              const float* Wv, const float* bv, int scale_mode,
                              float scale_a, const float* out, const float* m,
                              const float* z, const float* gout, float* gqkv,
                              float* gedge_attr, int gedge_attr_accumulate, float* gWk,
                              float* gbk, float* gWq, float* gbq, float* gWv, float* gbv,
                              void* ws, size_t ws_bytes, spt_stream_t stream);

/* The mode word.  The *_ex / *_m entries take a `mode` word that carries the formulation per call:
 *   bits 0-1  precision: SPT_ATTN_VALU 0, SPT_ATTN_F32 1 (f32 matrix pipe), SPT_ATTN_SPLIT_BF16 2,
 *             SPT_ATTN_BF16 3 (operands rounded to bf16);
 *   bits 4-5  backward form of the bf16-pipe precisions: 0 open, SPT_ATTN_BWD_PER_NODE,
 *             SPT_ATTN_BWD_PACKED, SPT_ATTN_BWD_EDGE_LANE;
 *   bits 6-7  edge order of the edge-lane backward: 0 open, SPT_ATTN_BWD_TARGET_ORDER
 *             (csrc/edge_attn_to.hip: dk / dv reduced per target inside the tile, a few float
 *             atomics per node - the sums' order, not their value, varies run to run),
 *             SPT_ATTN_BWD_SOURCE_ORDER (csrc/edge_attn_el.hip: no atomics, every gradient
 *             bitwise reproducible).
 * mode < 0 (SPT_ATTN_DEFAULT) leaves all three fields open.  An OPEN field is filled from the
 * process defaults (spt_attn_use_mfma, spt_attn_bwd_packed, spt_attn_bwd_el_target_order) at the
 * moment of the call.  spt_attn_resolve_mode(mode) does that and returns the fully explicit word:
 * it is the one function of the library that reads those three switches, every entry that takes
 * a mode word resolves it once on entry and works on the result, and a caller that resolves the
 * word itself and hands the result to every later call (forward, tile records, backward) is
 * independent of the switches from then on - two callers (two models at different precisions,
 * two streams) never change each other's arithmetic.  The resolver marks the fields IT filled in
 * (SPT_ATTN_FORM_OPEN, SPT_ATTN_ORDER_OPEN): such a field is a preference, one the caller wrote is
 * a demand (below).  Resolving is idempotent; bits outside the fields and marks are dropped.
 *
 * Route of the backward (spt_edge_attn_bwd_ex_f32), from the resolved word (precision p, form,
 * order), the shape and the operands the caller hands over.  "Built shape" = H 16, D 4, Dv 4, F 32
 * with edge_attr and all three encoders; tables = spt_edge_attn_bwd_workspace_bytes; ex =
 * tables + the scratch of the edge order in question (spt_edge_attn_bwd_ex_workspace_bytes covers
 * both orders).
 *   VALU     p == 0, or not the built shape: the generic lane-per-output kernels (a shape outside
 *            their compiled cases returns -4; without edge_attr F counts as 32);
 *   TARGET   form edge lane, p >= 2, e > 0, order target, src_sorted given, the target view
 *            (tperm, trowptr) or target-order tile_ids given, ws_bytes >= ex: csrc/edge_attn_to.hip;
 *   SOURCE   form edge lane, p >= 2, e > 0, not TARGET, the target view given, ws_bytes >= ex:
 *            csrc/edge_attn_el.hip;
 *   PACKED   none of the above, p >= 2, form not per node, e > 0: packed tiles over the edge stream;
 *   PER_NODE everything else on the built shape (p == 1 - the only f32-pipe backward -, form per
 *            node, e == 0): one tile set per source node.
 * The downgrades of an open field are silent, and these are all of them:
 *   order target -> SOURCE   src_sorted missing or ws_bytes below the target order's need, with
 *                            the view given (tile_ids, being target-order records, are ignored and
 *                            rebuilt in the workspace - no kernel reads records of the other format);
 *   edge lane -> PACKED      no view and no usable records, or ws_bytes below the order's need;
 *   edge lane -> PER_NODE    p == 1, or e == 0;
 *   packed -> PER_NODE       p == 1, or e == 0.
 * A field the CALLER wrote refuses instead (-1), on the built shape with p != 0: SPT_ATTN_BWD_EDGE_LANE
 * when the route is neither TARGET nor SOURCE; SPT_ATTN_BWD_TARGET_ORDER when an edge-lane route is
 * possible (form edge lane, p >= 2, e > 0, view or records + src_sorted) but TARGET is not.  tperm
 * and trowptr come both or neither.  VALU, PER_NODE and PACKED zero gqkv first (they add into it).
 * spt_edge_attn_bwd_route answers the same question without launching anything - the entry
 * itself switches on the same function's result: `operands` = SPT_ATTN_HAS_* of what the call will
 * be given (SPT_ATTN_HAS_RPE: edge_attr and all three encoders; F <= 0: no edge_attr), the result
 * one of SPT_ATTN_ROUTE_* or the negative status the launch would return (spt_last_error() set).
 *
 * Edge-lane backward (csrc/edge_attn_el.hip; H=16, D=Dv=4, F=32): 16-edge tiles over the CSR edge
 * stream, a wave owns half of the heads; the recompute GEMM runs transposed so that a lane holds
 * whole heads of ONE edge (no redundant softmax math, per-edge node rows fetched by LDS-DMA, any
 * number of source nodes per tile), dq is reduced per source node on the matrix pipe, two waves
 * per SIMD.  dk / dv are NOT scattered with atomics (the chip retires ~320 G f32 atomic adds / s:
 * 2.8 ms for one level-1 call): the per-edge [dk | dv] rows are streamed to the workspace in CSR
 * order and summed per target through (tperm, trowptr) = spt_csr_build(tgt_sorted, e, n) - a CSR
 * view of the TARGETS over the CSR positions, built once per batch and level - in a fixed order
 * (deterministic); dq of a node whose edges lie in several tiles is summed in ascending tile order
 * by the same pass (two 256 B slots per tile), so no sum depends on the order the waves run in.
 * It needs the scratch of spt_edge_attn_bwd_ex_workspace_bytes(n, e, ...)
 * (per-node rows + 512 B per edge + 512 B per tile), that view, and optionally src_sorted [e] int32 =
 * edge_index[0] in CSR order (NULL: rebuilt from erowptr).
 * With gedge_attr_accumulate == 0 the edge-lane kernel zero-fills gedge_attr first (both waves of
 * a pair add their halves). */
#define SPT_ATTN_DEFAULT (-1)
#define SPT_ATTN_VALU 0
#define SPT_ATTN_F32 1
#define SPT_ATTN_SPLIT_BF16 2
#define SPT_ATTN_BF16 3
#define SPT_ATTN_BWD_PER_NODE (1 << 4)
#define SPT_ATTN_BWD_PACKED (2 << 4)
#define SPT_ATTN_BWD_EDGE_LANE (3 << 4)
#define SPT_ATTN_BWD_TARGET_ORDER (1 << 6)
#define SPT_ATTN_BWD_SOURCE_ORDER (2 << 6)
#define SPT_ATTN_FORM_OPEN (1 << 8)  /* set by the resolver: bits 4-5 hold the process default */
#define SPT_ATTN_ORDER_OPEN (1 << 9) /* set by the resolver: bits 6-7 hold the process default */
int spt_attn_resolve_mode(int mode);
#define SPT_ATTN_HAS_RPE 1
#define SPT_ATTN_HAS_SRC 2
#define SPT_ATTN_HAS_TILE_IDS 4
#define SPT_ATTN_HAS_TARGET_VIEW 8
#define SPT_ATTN_ROUTE_VALU 0
#define SPT_ATTN_ROUTE_PER_NODE 1
#define SPT_ATTN_ROUTE_PACKED 2
#define SPT_ATTN_ROUTE_EDGE_LANE_SOURCE 3
#define SPT_ATTN_ROUTE_EDGE_LANE_TARGET 4
int spt_edge_attn_bwd_route(int64_t n, int64_t e, int H, int D, int Dv, int F, int operands, int mode,
                            size_t ws_bytes);
int spt_edge_attn_fwd_ex_f32(const float* qkv, int64_t n, int H, int D, int Dv,
                             const int32_t* erowptr, const int32_t* eperm,
                             const int32_t* tgt_sorted, int64_t e,
                             const float* edge_attr, int F, const float* Wk,
                             const float* bk, const float* Wq, const float* bq,
                             const float* Wv, const float* bv, int scale_mode,
                             float scale_a, float* out, float* m, float* z, int mode,
                             spt_stream_t stream);
/* Scratch for either edge order of the edge-lane backward (the larger of the two layouts: the
 * target order needs 644 B per node + 256 B per edge + 16 B per tile id, the source order
 * 388 B per node + 516 B per edge + 12 B per tile id) on top of the weight-gradient tables. */
size_t spt_edge_attn_bwd_ex_workspace_bytes(int64_t n, int64_t e, int H, int D, int Dv, int F);
/* 1 when the edge-lane backward is built for this head layout AND the resolved `mode` selects it
 * (form edge lane, a bf16-pipe precision). */
int spt_edge_attn_bwd_el_supported(int H, int D, int Dv, int F, int mode);
/* [ceil(e / 16)][48] int32 tile records of the edge-lane backward (edge rows | targets | sources of
 * 16 consecutive CSR positions): depends on the graph only, built once per batch and level by the
 * caller (tile_ids = NULL: rebuilt in the workspace on every call). */
int spt_attn_pack_tile_ids(const int32_t* eperm, const int32_t* tgt_sorted,
                           const int32_t* src_sorted, int64_t e, int32_t* tile_ids,
                           spt_stream_t stream);
int spt_edge_attn_bwd_ex_f32(const float* qkv, int64_t n, int H, int D, int Dv,
                             const int32_t* erowptr, const int32_t* eperm,
                             const int32_t* tgt_sorted, const int32_t* src_sorted,
                             const int32_t* tile_ids, const int32_t* tperm,
                             const int32_t* trowptr, int64_t e, const float* edge_attr, int F,
                             const float* Wk,
                             const float* bk, const float* Wq, const float* bq,
                             const float* Wv, const float* bv, int scale_mode,
                             float scale_a, const float* out, const float* m,
                             const float* z, const float* gout, float* gqkv,
                             float* gedge_attr, int gedge_attr_accumulate, float* gWk,
                             float* gbk, float* gWq, float* gbq, float* gWv, float* gbv,
                             int mode, void* ws, size_t ws_bytes, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Radius-bounded exact kNN on a uniform grid                        (a9)
 * Replaces frnn.frnn_grid_points of the un-vendored FRNN CUDA extension
 * (src/utils/neighbors.py:48 <- knn_1 :90, knn_2 :231): for each query the K
 * nearest search points with squared distance < r^2 (<= when inclusive),
 * ascending by (distance, index) - ties broken by ascending search index -,
 * missing entries idx = -1 / dist = -1.  d2 = (dx*dx + dy*dy) + dz*dz in f32.
 *   query [nq,3], search [ns,3] f32; K in [1,64]; idx [nq,K] int64,
 *   dist [nq,K] f32 (squared when `squared`, FRNN's convention, else Euclidean);
 *   cell_size/origin[3]/dims[3]: HOST description of the uniform grid that
 *   covers the search points (any cell size gives the same result; ~K/4 points
 *   per non-empty cell is fastest); dims[0]*dims[1]*dims[2] < 2^31;
 *   order_queries_by_cell: when query == search, visit queries in cell order.
 *   cell_order (nullable) [ns] int32: receives the search points' cell order (the
 *   permutation spt_spatial_order computes), a by-product of the grid build.
 * ws: spt_grid_knn_workspace_bytes(ns, ncells).
 * ---------------------------------------------------------------------- */
size_t spt_grid_knn_workspace_bytes(int64_t ns, int64_t ncells);
/* A self-search visited in cell order (query == search, order_queries_by_cell) has two
 * equivalent implementations: waves that own 64 consecutive cell-sorted points and share
 * one candidate stream (default), and one wave per query (also the path of every other
 * call).  spt_knn_use_cell_path(0|1) selects process-wide and returns the previous
 * setting; tests cross-check the two bit for bit. */
int spt_knn_use_cell_path(int on);
/* spt_grid_knn_f32 with the formulation chosen per call (-1: process default, 0: one wave per
 * query, 1: cell-centric self-search where it applies). */
int spt_grid_knn_ex_f32(const float* query, int64_t nq, const float* search, int64_t ns,
                        int K, float r, float cell_size, const float* origin,
                        const int32_t* dims, int order_queries_by_cell, int inclusive,
                        int squared, int64_t* idx, float* dist, int32_t* cell_order,
                        int formulation, void* ws, size_t ws_bytes, spt_stream_t stream);
/* KNN + PointFeatures of the reference's preprocessing chain in ONE call (src/transforms/
 * neighbors.py:11-95 -> src/transforms/point.py:160-180 -> src/utils/geometry.py:80-126): a
 * self-search of `xyz` [n, 3] for the K nearest of every point (itself included, column 0:
 * K = k + 1 of knn_1, K <= 64) that also writes feats [n, 11] = the eigenfeatures (pgeof's
 * column order) of each point's neighbourhood {found points} - what spt_point_geof_dense_f32
 * returns for (xyz, idx[:, 1:], add_self = 1, k_min, post), without the index rows and the
 * neighbours' positions coming back from HBM: the kNN kernel sums the f64 moments of the winners
 * while their rows are still in cache.  The summation order differs from the stand-alone entry:
 * results are identical whenever the sums are exact in f64 (coordinates of similar magnitude,
 * the usual case) and within an ulp of the f32 outputs otherwise.  idx / dist / cell_order /
 * formulation / ws as in spt_grid_knn_ex_f32 (the one-wave-per-query formulation computes the
 * features from the index rows it wrote). */
int spt_grid_knn_geof_f32(const float* xyz, int64_t n, int K, float r, float cell_size,
                          const float* origin, const int32_t* dims, int inclusive, int squared,
                          int k_min, int post, int64_t* idx, float* dist, float* feats,
                          int32_t* cell_order, int formulation, void* ws, size_t ws_bytes,
                          spt_stream_t stream);
/* Probes of the host-side grid description (which cell size makes the search fastest; the
 * RESULT of a search never depends on it).  spt_knn_subsample_f32: the points of the coarse cells
 * (edge `coarse`, origin lo[3] - HOST floats) whose coordinate hash & 0xFFFF is below `thresh`,
 * compacted into out [<= n, 3] in no particular order, their number in the DEVICE int32 *count.
 * spt_grid_cell_ids_f32: the linear cell id ((z * dims[1] + y) * dims[0] + x, clamped) of every
 * point for a grid description as in spt_grid_knn_f32. */
int spt_knn_subsample_f32(const float* xyz, int64_t n, const float* lo, float coarse, int thresh,
                          float* out, int32_t* count, spt_stream_t stream);
int spt_grid_cell_ids_f32(const float* xyz, int64_t n, float cell_size, const float* origin,
                          const int32_t* dims, int64_t* cell, spt_stream_t stream);
/* The number of non-empty cells of that grid in the DEVICE int64 *count (exact: one bit per cell,
 * set by the points, then counted - no sort).  ws: spt_grid_count_cells_workspace_bytes(ncells). */
size_t spt_grid_count_cells_workspace_bytes(int64_t ncells);
int spt_grid_count_cells_f32(const float* xyz, int64_t n, float cell_size, const float* origin,
                             const int32_t* dims, int64_t* count, void* ws, size_t ws_bytes,
                             spt_stream_t stream);
/* Bounding box of a cloud, the input of the host-side grid description above
 * (src/utils/neighbors.py has no counterpart: FRNN derives its grid internally).
 * lo_hi: DEVICE float[12]; [0..3) = min, [3..6) = max, [6..12) scratch. */
int spt_bbox_f32(const float* xyz, int64_t n, float* lo_hi, spt_stream_t stream);
int spt_grid_knn_f32(const float* query, int64_t nq, const float* search, int64_t ns,
                     int K, float r, float cell_size, const float* origin,
                     const int32_t* dims, int order_queries_by_cell, int inclusive,
                     int squared, int64_t* idx, float* dist, int32_t* cell_order, void* ws,
                     size_t ws_bytes, spt_stream_t stream);
/* Continuation of a search: for every query the K search points ranked strictly AFTER
 * (after_d2[q], after_idx[q]) in the contract's (squared distance, index) order - chained after a
 * K = 64 call it returns neighbours 65..128, which lifts the 64-per-call limit of the kernels
 * (cluster_radius_nn_graph's k_max = 100, src/utils/neighbors.py:491).  after_idx[q] < 0 = the
 * previous list was not full: nothing left (all -1).  after_d2 is SQUARED whatever `squared`. */
int spt_grid_knn_after_f32(const float* query, int64_t nq, const float* search, int64_t ns, int K,
                           float r, float cell_size, const float* origin, const int32_t* dims,
                           int inclusive, int squared, const int64_t* after_idx,
                           const float* after_d2, int64_t* idx, float* dist, void* ws,
                           size_t ws_bytes, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Point geometric features                                          (a11-a14)
 * Replaces pgeof.compute_features (src/utils/geometry.py:148-153) and the torch
 * branch the reference takes on GPU (_geometric_features_torch :236-338 +
 * scatter_pca, src/utils/scatter.py:41-125): per point the population
 * covariance of {self} + valid neighbours, its 3x3 eigen-decomposition and
 *   feats [n,11] = [linearity, planarity, scattering, verticality, nx, ny, nz,
 *                   length, surface, volume, curvature]   (geometry.py:165-174)
 * dense: nn [n,k] int64, negative = missing (FRNN padding); csr: nn_val / nn_ptr
 * [n+1] int64 (pgeof layout).  add_self: count the point itself (geometry.py:95-96);
 * features are zeroed where the neighbourhood has < k_min points; post != 0
 * applies geometric_features' tail (verticality * 2, normal flipped to z >= 0,
 * geometry.py:121,124).  order (nullable): a permutation of the points, e.g.
 * spt_spatial_order's; points are visited in that order so that the neighbourhoods a
 * wave gathers overlap (results do not depend on it).
 * spt_spatial_order: order[j] = j-th point when grouped by the cells of a uniform grid
 * (HOST cell_size / origin[3] / dims[3] as for spt_grid_knn_f32).
 * ---------------------------------------------------------------------- */
size_t spt_spatial_order_workspace_bytes(int64_t n, int64_t ncells);
int spt_spatial_order(const float* xyz, int64_t n, float cell_size, const float* origin,
                      const int32_t* dims, int32_t* order, void* ws, size_t ws_bytes,
                      spt_stream_t stream);
int spt_point_geof_dense_f32(const float* xyz, int64_t n, const int64_t* nn, int k,
                             int add_self, int k_min, int post, const int32_t* order,
                             float* feats, spt_stream_t stream);
/* The same with a row pitch: nn[i * ld + c], ld >= k - a column slice of a wider table (knn_1's
 * [N, k] result is columns 1 .. k of a [N, k + 1] search) is read in place. */
int spt_point_geof_dense_ld_f32(const float* xyz, int64_t n, const int64_t* nn, int k, int64_t ld,
                                int add_self, int k_min, int post, const int32_t* order,
                                float* feats, spt_stream_t stream);
int spt_point_geof_csr_f32(const float* xyz, int64_t n, const int64_t* nn_val,
                           const int64_t* nn_ptr, int add_self, int k_min, int post,
                           float* feats, spt_stream_t stream);
/* scatter_pca (src/utils/scatter.py:41-125, algorithm='eigh') as an entry of its own (a12):
 * for every group of the CSR view (perm nullable = rows already grouped) the population
 * covariance of x [rows, 3], its eigenvalues ascending and clamped at 0 -> eigenval [S,3],
 * eigenvectors in the COLUMNS of eigenvec [S,3,3] (torch.linalg.eigh's layout; the sign of a
 * column is arbitrary there as here); an empty group yields (1,1,1) / identity
 * (scatter.py:113-118). */
int spt_scatter_pca_f32(const float* x, const int32_t* perm, const int32_t* rowptr,
                        int64_t num_seg, float* eigenval, float* eigenvec, spt_stream_t stream);
/* neighbors_dense_to_csr (src/utils/neighbors.py:668-684)                       (a10)
 * nn [n,k] int64 with negative = missing -> ptr [n+1], val [capacity n*k, first ptr[n]
 * entries valid, row order kept], sizes [n] (all int64). */
size_t spt_neighbors_dense_to_csr_workspace_bytes(int64_t n);
int spt_neighbors_dense_to_csr(const int64_t* nn, int64_t n, int k, int64_t* ptr, int64_t* val,
                               int64_t* sizes, void* ws, size_t ws_bytes, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Per-segment random sampling without replacement                      (f2/f3)
 * Replaces sparse_sample (src/utils/sparse.py:142-243) behind NAG.get_sampling
 * (src/data/nag.py:672-711): shuffle + stable sort by segment + take the first
 * n_samples[s] of every segment, with
 *   n_samples = clamp(floor(n_max * tanh(size / n_max)), n_min, size)   (n_max > 0)
 *             = clamp(round(sqrt(size)), n_min, size)                   (n_max <= 0)
 * mask (nullable, 1 = keep): heuristic on the unmasked sizes, then clamped to the
 * number of kept elements (sparse.py:180-205).  out_ptr [num_seg+1] int64
 * (out_ptr[num_seg] = number of samples, never more than n), out_idx [n] int64 (only the
 * first out_ptr[num_seg] are written).
 *
 * The draw is a function of (idx, mask, n_max, n_min, seed) alone, specified to the bit
 * (rand32 = the splitmix64 finaliser of csrc/rng.hpp; restated on the host by
 * tests/sampling_reference.py, which tests/test_sampling_gpu.py holds the output to):
 *   key[i]    = rand32(seed, i)                                    i in [0, n)
 *   order1    = stable argsort of key, ascending, unsigned         (the shuffle)
 *   bucket[p] = idx[order1[p]]  if 0 <= idx < num_seg and (mask == NULL or mask[order1[p]])
 *               else num_seg                                       (tail bucket, never drawn)
 *   order2    = order1[stable argsort of bucket]
 *   kept[s]   = population of bucket s
 *   size[s]   = number of i with idx[i] == s (mask ignored) when a mask is given, else kept[s]
 *   cnt[s]    = min(max(heuristic(size[s]), n_min), size[s], kept[s])
 *   heuristic = floor(f32(n_max) * tanh_f32(f32(size) / f32(n_max)))          n_max > 0
 *             = round_half_even(sqrt_f32(f32(size)))                          n_max <= 0
 *               (tanh_f32 = the correctly rounded f32 value, which is what the reference's
 *               host evaluation gives over the whole saturation band)
 *   out_ptr   = exclusive cumsum of cnt, length num_seg + 1
 *   out_idx[out_ptr[s] + j] = order2[first position of bucket s + j]          j < cnt[s]
 * Rows whose idx lies outside [0, num_seg) are never drawn and never counted in size.
 * Equal keys (certain from about 1e5 elements on) keep ascending position: both sorts are
 * stable.
 * ---------------------------------------------------------------------- */
size_t spt_sparse_sample_workspace_bytes(int64_t n, int64_t num_seg);
int spt_sparse_sample(const int64_t* idx, int64_t n, int64_t num_seg, const uint8_t* mask,
                      int n_max, int n_min, uint64_t seed, int64_t* out_ptr,
                      int64_t* out_idx, void* ws, size_t ws_bytes, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Segment statistics of SegmentFeatures                                   (f2)
 * spt_segment_std_f32: torch_scatter.scatter_std(x, idx, dim=0) (unbiased, denominator
 *   max(cnt-1, 1) + 1e-6) as called at src/transforms/graph.py:285; x [n,c], out [num_seg,c].
 * spt_segment_mean_orientation_f32: scatter_mean_orientation
 *   (src/utils/scatter.py:249-300); orientation [n,3] -> out [num_seg,3] (unit, z >= 0).
 * Rows are visited through the CSR view (perm nullable = already grouped).
 * ---------------------------------------------------------------------- */
int spt_segment_std_f32(const float* x, const int32_t* perm, const int32_t* rowptr,
                        int64_t num_seg, int c, float* out, spt_stream_t stream);
int spt_segment_mean_orientation_f32(const float* orientation, const int32_t* perm,
                                     const int32_t* rowptr, int64_t num_seg, float* out,
                                     spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Radius graph between point clusters                                     (f2)
 * The two device-heavy stages of cluster_radius_nn_graph
 * (src/utils/neighbors.py:491-665).
 *
 * spt_cluster_graph_edges (:563-613): neighbours [S,k] int64 (-1 = missing) and
 *   distances [S,k] f32 of the cluster centres (knn_1's output), r_cluster [S] = diam/2;
 *   keeps `dist <= r_s + r_t + 1.732 * gap`, then to_trimmed (trim != 0: s < t,
 *   src/utils/graph.py:466-502) or coalesce, both with reduce = 'min', no self loops.
 *   edges [2, S*k] int64 (row stride S*k), edge_dist [S*k]: the first *count columns are
 *   written, sorted by (s, t); count: device int64.
 *
 * spt_cluster_pair_anchors_f32: scatter_nearest_neighbor (src/utils/scatter.py:128-238)
 *   + anchor distance (neighbors.py:631-632) for every edge (s, t): `cycles` rounds of
 *   "closest point of t to s's candidate, closest point of s to t's candidate" starting
 *   from the cluster centroids [S,3]; clusters are walked through the CSR view
 *   (perm, rowptr) of the point -> cluster index; ties -> first point in CSR order.
 *   edges: row 0 at edges[0..E), row 1 at edges[edge_stride..]; anchors [2,E] int64 point
 *   indices, d_nn [E].  group_lanes in {8,16,64}: lanes cooperating on one edge.
 * ---------------------------------------------------------------------- */
size_t spt_cluster_graph_edges_workspace_bytes(int64_t num_clusters, int k);
int spt_cluster_graph_edges(const int64_t* neighbors, const float* distances,
                            const float* r_cluster, int64_t num_clusters, int k, float gap,
                            int trim, int64_t* edges, float* edge_dist, int64_t* count,
                            void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_cluster_pair_anchors_f32(const float* points, const int32_t* perm, const int32_t* rowptr,
                                 const float* centroid, const int64_t* edges, int64_t num_edges,
                                 int64_t edge_stride, int cycles, int group_lanes,
                                 int64_t* anchors, float* d_nn, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Input graph of the partition, from the kNN table
 * AdjacencyGraph(k, w)._process (src/transforms/graph.py:67-96), Data.connect_isolated
 * (src/data/data.py:481-561; isolated_nodes, src/utils/graph.py:44-53), Data.to_trimmed
 * (data.py:563-586; src/utils/graph.py:466-502) and the forward star of the sorted edges
 * (src/transforms/partition.py:190-196), without the edge list, its unique() and the
 * coalesce sort: the mirror of entry i -> j is one of the first k entries of row j.
 *
 * neighbors [n, ld] int64 (any negative entry = missing), distances [n, ld] f32 (nullable
 * when w <= 0); the first k <= min(ld, 64) columns are read in place.  n < 2^31.
 *
 * spt_adjacency_stats: linked [n] u8 = 1 for every source and every target of a directed
 *   edge (graph.py:44-53 negated); stats: 4 device doubles = number of valid entries, sum of
 *   their distances (f64; mean of graph.py:92), number of isolated nodes, flag word (1: a row
 *   names a node twice among its first k entries - the entries below do not apply, 2: an
 *   entry >= n).
 * spt_adjacency_regression: sums: 4 device doubles = sum d, sum d^2, sum wgt, sum d wgt over
 *   the valid entries, d = |pos_i - pos_j|, wgt = 1 / (w + dist / mean) or 1 (w <= 0): with
 *   the entry count, the normal equations of the lstsq of data.py:535-545.  Workspace: the
 *   one of spt_adjacency_stats.
 * spt_adjacency_count: the isolated nodes' new edges (data.py:519-524) are extra rows:
 *   node iso_index[q] (ascending), entries iso_neighbors [num_isolated, k_isolated].  An entry
 *   i -> j, j != i, survives iff i < j or node j does not list i.  keep [n + num_isolated]:
 *   one bit per column; row_start [n + 1] u32: first output slot of every smaller end point,
 *   row_start[n] = number of edges.
 * spt_adjacency_fill: edge_index [2, num_edges] int64 sorted by (i, j), i < j (coalesce's
 *   order); edge_attr [num_edges] f32 (nullable: no weights) - both directions of a pair
 *   merged with reduce (0 mean, 1 add, 2 min, 3 max), the extra rows' weights given in
 *   iso_weights [num_isolated, k_isolated] (data.py:556); source_csr [n + 1] int64.
 *   Bitwise reproducible.
 * ---------------------------------------------------------------------- */
size_t spt_adjacency_stats_workspace_bytes(int64_t num_nodes);
int spt_adjacency_stats(const int64_t* neighbors, const float* distances, int64_t num_nodes,
                        int64_t ld, int k, uint8_t* linked, double* stats, void* ws,
                        size_t ws_bytes, spt_stream_t stream);
int spt_adjacency_regression(const int64_t* neighbors, const float* distances, const float* pos,
                             int64_t num_nodes, int64_t ld, int k, float w, float mean,
                             double* sums, void* ws, size_t ws_bytes, spt_stream_t stream);
size_t spt_adjacency_count_workspace_bytes(int64_t num_nodes);
int spt_adjacency_count(const int64_t* neighbors, int64_t num_nodes, int64_t ld, int k,
                        const uint8_t* linked, const int64_t* iso_index,
                        const int64_t* iso_neighbors, int64_t num_isolated, int k_isolated,
                        uint64_t* keep, uint32_t* row_start, void* ws, size_t ws_bytes,
                        spt_stream_t stream);
size_t spt_adjacency_fill_workspace_bytes(int64_t num_nodes, int64_t num_edges);
int spt_adjacency_fill(const int64_t* neighbors, const float* distances, int64_t num_nodes,
                       int64_t ld, int k, float w, float mean, const uint8_t* linked,
                       const int64_t* iso_index, const int64_t* iso_neighbors,
                       const float* iso_weights, int64_t num_isolated, int k_isolated, int reduce,
                       const uint64_t* keep, const uint32_t* row_start, int64_t num_edges,
                       int64_t* edge_index, float* edge_attr, int64_t* source_csr, void* ws,
                       size_t ws_bytes, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * GroundElevation: ground filters, RANSAC plane, elevation
 * GroundElevation._process (src/transforms/point.py:268-326) with model 'ransac': the three
 * filters of src/utils/ground.py:25-97 (xy_partition: src/utils/partition.py:17-50), the plane
 * of single_plane_model's CPU branch (ground.py:116-131: RANSACRegressor(residual_threshold) on
 * (xy, z), vertical residual, final least-squares fit on the inliers) and the elevation.
 * pos [n, 3] f32, one cloud, 1 <= n < 2^31.
 *
 * spt_ground_bounds_f32: bounds = 5 device floats: min z, then min and max of trunc(x / grid)
 *   and min and max of trunc(y / grid) (whole numbers; IEEE f32 division, truncation toward
 *   zero, exactly torch's div(..., rounding_mode='trunc')); grid <= 0: min z only, the rest 0.
 * spt_ground_cell_min_f32: table [num_i * num_j] u64, cell (i - i_min) * num_j + (j - j_min):
 *   (order-preserving bits of z) << 32 | index of the lowest point of the cell, all ones for an
 *   empty cell; among equal z (-0.0 == +0.0) the lowest index wins.  Every point takes part
 *   (ground.py:45-71 runs on the whole cloud).  A point outside the table is skipped.
 * spt_ground_trim_f32: index [capacity] int64 = the points with z - bounds[0] < z_threshold
 *   (use_z) and verticality < verticality_threshold (verticality [n] non-NULL) that are the
 *   winner of their cell (table non-NULL), in increasing point order; *count (device int64) =
 *   their number M, never above capacity.  ws: spt_ground_trim_workspace_bytes(n).
 * spt_ground_ransac_f32: num_hypotheses <= 256 triplets of trimmed points, either
 *   idx = min(floor(u M), M - 1) from u [H, 3] f32 in [0, 1) or samples [H, 3] int64 given
 *   (exactly one non-NULL); M = *count is read on the device.  counts [H] int32 = number of
 *   trimmed points with |z - (a x + b y + c)| < residual_threshold for the plane through the
 *   triplet (f64 arithmetic), -1 for a triplet with a repeated or out-of-range index or a
 *   triangle degenerate in XY.  status = 8 device doubles: M, best count, best hypothesis
 *   (largest count, lowest index among equals; -1: none valid), a, b, c of the least-squares
 *   plane of the best hypothesis's inliers (f64 moments, per-workgroup partials summed in a
 *   fixed order), number of valid hypotheses, number of inliers refitted (-1: inliers
 *   rank-deficient, (a, b, c) is the hypothesis's own plane).  Bitwise reproducible.
 * spt_ground_elevation_f32: elevation [n] = (z - (a x + b y + c)) / scale, plane read from
 *   status on the device, f64 arithmetic rounded once.
 * ---------------------------------------------------------------------- */
size_t spt_ground_bounds_workspace_bytes(int64_t num_points);
int spt_ground_bounds_f32(const float* pos, int64_t num_points, float grid, float* bounds,
                          void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_ground_cell_min_f32(const float* pos, int64_t num_points, float grid, int64_t i_min,
                            int64_t j_min, int64_t num_i, int64_t num_j, uint64_t* table,
                            spt_stream_t stream);
size_t spt_ground_trim_workspace_bytes(int64_t num_points);
int spt_ground_trim_f32(const float* pos, int64_t num_points, const float* bounds, int use_z,
                        float z_threshold, const float* verticality, float verticality_threshold,
                        const uint64_t* table, int64_t num_cells, int64_t* index,
                        int64_t capacity, int64_t* count, void* ws, size_t ws_bytes,
                        spt_stream_t stream);
size_t spt_ground_ransac_workspace_bytes(int num_hypotheses);
int spt_ground_ransac_f32(const float* pos, int64_t num_points, const int64_t* index,
                          const int64_t* count, int64_t capacity, const float* u,
                          const int64_t* samples, int num_hypotheses, double residual_threshold,
                          int32_t* counts, double* status, void* ws, size_t ws_bytes,
                          spt_stream_t stream);
int spt_ground_elevation_f32(const float* pos, int64_t num_points, const double* status,
                             float scale, float* elevation, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * PointFeatures: colour keys and density                  (csrc/point_feat.hip)
 * PointFeatures._process (src/transforms/point.py:116-182): to_float_rgb (src/utils/color.py:
 * 17-22), rgb2hsv and rgb2lab (src/utils/features.py:8-86) with the / 360 of the hue and the
 * / 100 of lab, and density = k_n / dmax_n^2 (point.py:158-161).
 *
 * spt_point_color_f32: rgb [n, 3] contiguous, uint8 (rgb_is_u8) or f32.  keys: bit 0 rgb as
 *   [0, 1] floats, bit 1 hsv, bit 2 lab; each selected output is [n, 3] f32 written at
 *   out[i * ld + c], c < 3: ld = 3 for a tensor of its own, ld = F and out = table + column for
 *   a block of a wider [n, F] table.  The values do not depend on ld or on alignment.  The
 *   colours are divided by 255 when some value is > 1 (decided on the device, no host read;
 *   a NaN anywhere: not divided, as rgb.max() > 1 is False) and clamped to [0, 1].  hsv: the
 *   reference's f32 operations in its order, IEEE division; hue = (h2, h3, h1)[argmin], first
 *   minimal channel on ties, / 360 (grey 0.5, [9, 5, 5] 1.0, black s = 1).  lab: sRGB
 *   linearisation (accurate powf), x 100, matrix, round to 4 decimals, white point, cbrtf or
 *   the linear branch, second matrix, L - 16, round to 4 decimals, / 100.  An output must not
 *   overlap rgb.  ws: spt_point_color_workspace_bytes(n), 4-byte aligned.
 * spt_point_density_f32: density [n] f32 = float(count of neighbor_index[i, :k] >= 0) /
 *   (max of neighbor_distance[i, :k])^2, plain IEEE f32 (all distances -1: 0 / 1 = 0; max 0:
 *   inf; a NaN distance: NaN).  Row i of a table starts at element i * ld (ld >= k): a column
 *   slice of a wider table is read in place.  1 <= k <= 255.
 * n = 0 returns 0 without a launch.
 * ---------------------------------------------------------------------- */
size_t spt_point_color_workspace_bytes(int64_t num_points);
int spt_point_color_f32(const void* rgb, int rgb_is_u8, int64_t num_points, int keys,
                        float* out_rgb, int64_t ld_rgb, float* out_hsv, int64_t ld_hsv,
                        float* out_lab, int64_t ld_lab, void* ws, size_t ws_bytes,
                        spt_stream_t stream);
int spt_point_density_f32(const int64_t* neighbor_index, int64_t ld_index,
                          const float* neighbor_distance, int64_t ld_distance,
                          int64_t num_points, int k, float* density, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * NAG selection / re-indexing                                             (f3)
 * The integer work of NAG.select (src/data/nag.py:306-399), Data.select
 * (src/data/data.py:286-470) and Cluster.select (src/data/cluster.py:79-140).  All ids
 * are bounded by a level size, so every consecutive_cluster (torch.unique) of the
 * reference is a presence bitmap + scan here.  Counts are device int64 scalars.
 *
 * spt_index_inverse: inv [n] = -1 except inv[idx[j]] = j          (data.py:365-368)
 * spt_select_edges: edges whose two ends survive, relabelled through inv, original
 *   order kept; idx_edge = their positions (data.py:369-373).  edge_index rows at
 *   [0..E) and [edge_stride..); out rows at [0..) and [out_stride..).
 * spt_cluster_select: clusters idx [k] (no duplicates) of the CSR (pointers [S+1],
 *   points [num_points], point ids < n_sub) -> new_pointers [k+1], new_points (dense
 *   new ids, first new_pointers[k] entries), idx_sub (ascending surviving point ids,
 *   first *count_sub entries) and sub_super (new cluster of each surviving point)
 *   (src/data/csr.py:328-408, cluster.py:127-138).
 * spt_relabel_consecutive: consecutive_cluster of values[gather[i]] (gather nullable)
 *   for labels in [0, n_range): new_values [k] dense labels in sorted order, uniques =
 *   the labels present, ascending (data.py:404-406: new super_index / idx_super).
 * spt_radius_ball_f32: ascending indices of the nodes within r of `center` (HOST float[3];
 *   z ignored when cylindrical) and of batch item `batch_id` (batch nullable) - the seed
 *   neighbourhood of SampleRadiusSubgraphs (src/transforms/sampling.py:1196-1230, via
 *   knn_brute_force, src/utils/neighbors.py:245-295: Euclidean norm, d <= r kept).
 * ---------------------------------------------------------------------- */
int spt_index_inverse(const int64_t* idx, int64_t k, int64_t n, int64_t* inv,
                      spt_stream_t stream);
size_t spt_select_edges_workspace_bytes(int64_t num_edges);
int spt_select_edges(const int64_t* edge_index, int64_t num_edges, int64_t edge_stride,
                     const int64_t* inv, int64_t n, int64_t* out_edges, int64_t out_stride,
                     int64_t* idx_edge, int64_t* count, void* ws, size_t ws_bytes,
                     spt_stream_t stream);
size_t spt_cluster_select_workspace_bytes(int64_t k, int64_t num_points, int64_t n_sub);
int spt_cluster_select(const int64_t* pointers, const int64_t* points, int64_t num_points,
                       const int64_t* idx, int64_t k, int64_t n_sub, int64_t* new_pointers,
                       int64_t* new_points, int64_t* idx_sub, int64_t* sub_super,
                       int64_t* count_sub, void* ws, size_t ws_bytes, spt_stream_t stream);
size_t spt_radius_ball_workspace_bytes(int64_t n);
int spt_radius_ball_f32(const float* pos, int64_t n, const float* center, float r,
                        int cylindrical, const int64_t* batch, int64_t batch_id,
                        int64_t* out_idx, int64_t* count, void* ws, size_t ws_bytes,
                        spt_stream_t stream);
size_t spt_relabel_consecutive_workspace_bytes(int64_t n_range);
int spt_relabel_consecutive(const int64_t* values, const int64_t* gather, int64_t k,
                            int64_t n_range, int64_t* new_values, int64_t* uniques,
                            int64_t* count, void* ws, size_t ws_bytes, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * On-the-fly horizontal edge features + symmetrisation + self loops   (f1)
 * Replaces _on_the_fly_horizontal_edge_features (src/transforms/graph.py:1135-1277,
 * all default keys) followed by NAGAddSelfLoops (:1419-1452).
 *   se [2,e] int64 trimmed edges (row-major: sources then targets);
 *   edge_attr7 [e,7] f32 = [mean_off(3), std_off(3), mean_dist];
 *   pos, normal [n,3]; log_length / log_surface / log_volume / log_size [n];
 *   edge_index_out [2, 2e (+n)] int64 = [(s,t) | (t,s) | (i,i)];
 *   edge_attr_out [2e (+n), 18] f32 in the reference's f_list column order;
 *   self-loop rows are zero.
 * ---------------------------------------------------------------------- */
int spt_horizontal_edge_features_f32(
    const int64_t* se, int64_t e, int64_t n, const float* edge_attr7, const float* pos,
    const float* normal, const float* log_length, const float* log_surface,
    const float* log_volume, const float* log_size, int add_self_loops,
    int64_t* edge_index_out, float* edge_attr_out, spt_stream_t stream);
/* On-the-fly VERTICAL edge features (src/transforms/graph.py:1335-1416, all default keys), one
 * row per child node with parent p = super_index[i]:
 *   [centroid_dir (3, 0/0 -> 0, clipped to [-1,1]), sqrt(centroid_dist), |<n_i, n_p>|,
 *    log_length_p - log_length_i, log_surface.., log_volume.., log_size..]      out [n, 9]. */
int spt_vertical_edge_features_f32(
    const int64_t* super_index, int64_t n, const float* child_pos, const float* child_normal,
    const float* child_log_length, const float* child_log_surface, const float* child_log_volume,
    const float* child_log_size, const float* parent_pos, const float* parent_normal,
    const float* parent_log_length, const float* parent_log_surface,
    const float* parent_log_volume, const float* parent_log_size, float* v_edge_attr,
    spt_stream_t stream);
/* Symmetric edge features of the panoptic edge-affinity head (src/models/panoptic.py:477-480):
 *   out[e] = cat(|x[a_e] - x[b_e]|, (x[a_e] + x[b_e]) / 2)   x [n,C], C % 4 == 0, out [e,2C].
 * Backward: gend [2e, C], row e = gradient reaching x[a_e] through edge e, row e + E the one
 * reaching x[b_e]; the caller sums them per node with spt_segcsr_reduce_f32 over cat(a, b). */
int spt_edge_affinity_features_f32(const float* x, int64_t n, int C, const int64_t* edge_a,
                                   const int64_t* edge_b, int64_t e, float* out,
                                   spt_stream_t stream);
int spt_edge_affinity_features_bwd_f32(const float* x, const float* gout, int64_t n, int C,
                                       const int64_t* edge_a, const int64_t* edge_b, int64_t e,
                                       float* gend, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Tall-skinny Linear: y [rows, N] = x [rows, K] W[N, K]^T (+ bias [N] or NULL), f32 in /
 * f32 accumulate.  The qkv / out_proj nn.Linear of SelfAttentionBlock
 * (src/nn/attention.py:202-215, 311-313) and, on (gy, W^T), their input gradients.
 * K in {32, 64, 128, 192} and - round 5 - 256 (the dX of the 128-wide blocks' qkv Linear) and
 * 132 / 260: the first Linear of the KITTI-360 width's
 * node MLPs ([4 + 128, 128, 128] / [4 + 256, 128, 128], configs/experiment/semantic/kitti360.yaml:
 * 22-27, src/nn/mlp.py:43-56), which ran on the vendor GEMM before.  N any width from 64 up (a last
 * slab of fewer than 64 columns - the dX of a 132 / 260-wide input - reads the missing weight rows
 * as zero and stores nothing for them), or N <= 16 (the heads); x, W, y contiguous.
 * ---------------------------------------------------------------------- */
int spt_skinny_linear_supported(int K, int N);
int spt_skinny_linear_f32(const float* x, int64_t rows, int K, const float* W, const float* bias,
                          int N, float* y, spt_stream_t stream);
/* Round 6: y [rows, N] = x [rows, K] Wt [K, N] - the same product with the weight given as the
 * TRANSPOSE of what spt_skinny_linear_f32 takes: the input gradient dX = G W of a Linear reads the
 * layer's own weight W [N_out = K, N_in = N] (what autograd of src/nn/attention.py:202-215 /
 * src/nn/mlp.py:43-56 computes) instead of a transposed copy made per backward call.  Same K as
 * above, N % 4 == 0 and N >= 64, Wt 16-byte aligned; no bias. */
int spt_skinny_linear_wt_f32(const float* x, int64_t rows, int K, const float* Wt, int N, float* y,
                             spt_stream_t stream);
/* Weight gradient of the same Linear: gw[N,K] = gy[rows,N]^T x[rows,K] (src/nn/attention.py's qkv /
 * out_proj under autograd), a reduction over 10^5..10^7 rows.  K in {32, 64, 128, 132, 260} (above
 * 64: 64-column slabs of x, the last one narrower), N a multiple of 64;
 * f32 in / f32 accumulate on the matrix pipe, per-wave partials summed in a fixed order
 * (deterministic).  gb[N] (nullable) receives the column sums of gy - the bias gradient - from the
 * same pass.  ws: spt_skinny_dw_workspace_bytes(K, N) bytes of device scratch. */
/* The transformer block's pre-norm and residual folded into its two Linears
 * (x = x + out_proj(attention(qkv(norm(x)))), src/nn/transformer.py:231-234):
 *   pre_am / pre_scale [num_graphs, K], pre_bias [K]: x_n = (x - pre_am[g]) * pre_scale[g] +
 *     pre_bias with g = batch[row] (batch NULL = one graph) applied while the rows are read - the
 *     tables of spt_graphnorm_stats_f32; pre_am NULL = plain x;
 *   residual [rows, N] or NULL: y = (x W^T + b) + residual.
 * K in {32, 64, 128}, N a multiple of 64, num_graphs * K <= 1024 (spt_skinny_pre_supported). */
int spt_skinny_pre_supported(int K, int N, int num_graphs);
int spt_skinny_linear_pre_f32(const float* x, int64_t rows, int K, const float* W, const float* bias,
                              int N, float* y, const float* pre_am, const float* pre_scale,
                              const float* pre_bias, const int64_t* batch, int num_graphs,
                              const float* residual, spt_stream_t stream);
/* gw = gy^T norm(x) (+ gb): the weight gradient of the Linear above (same tables). */
int spt_skinny_dw_pre_f32(const float* gy, const float* x, int64_t rows, int N, int K, float* gw,
                          float* gb, const float* pre_am, const float* pre_scale,
                          const float* pre_bias, const int64_t* batch, int num_graphs, void* ws,
                          size_t ws_bytes, spt_stream_t stream);
/* Round 6: matrix mode of the tall-skinny Linears (K = 32 / 64 and the K = 192 input gradient; the
 * other widths stay on the f32 pipe in every mode).  They ran on v_mfma_f32_16x16x4_f32 in every
 * mode; like the attention and the fused layers they now follow the mode the reference ships
 * (configs/train.yaml:60-61 float32_matmul_precision: high):
 *   0  f32 pipe (the f32-exact mode)
 *   1  (default) split bf16: the forward as the f32-EXACT six-product 3-way split, the input and
 *      weight gradients as hi*hi + lo*hi + hi*lo (three products)
 *   3  operands rounded to bf16 (the bf16 mode)
 * spt_skinny_use_split_bf16 sets the process-wide default and returns the previous one (< 0: query);
 * the _m entries take the mode per call (< 0: that default).  _pre_m = spt_skinny_linear_pre_f32 (a
 * forward: pre-norm / residual options), _wt_m = spt_skinny_linear_wt_f32 (an input gradient),
 * _dw_pre_m = spt_skinny_dw_pre_f32 (a weight gradient). */
int spt_skinny_use_split_bf16(int mode);
int spt_skinny_linear_pre_m_f32(const float* x, int64_t rows, int K, const float* W, const float* bias,
                                int N, float* y, const float* pre_am, const float* pre_scale,
                                const float* pre_bias, const int64_t* batch, int num_graphs,
                                const float* residual, int mode, spt_stream_t stream);
int spt_skinny_linear_wt_m_f32(const float* x, int64_t rows, int K, const float* Wt, int N, float* y,
                               int mode, spt_stream_t stream);
int spt_skinny_dw_pre_m_f32(const float* gy, const float* x, int64_t rows, int N, int K, float* gw,
                            float* gb, const float* pre_am, const float* pre_scale,
                            const float* pre_bias, const int64_t* batch, int num_graphs, int mode,
                            void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_skinny_dw_supported(int K, int N);
size_t spt_skinny_dw_workspace_bytes(int K, int N);
int spt_skinny_dw_f32(const float* gy, const float* x, int64_t rows, int N, int K, float* gw,
                      float* gb, void* ws, size_t ws_bytes, spt_stream_t stream);
/* One-pass backward of y = x W^T + b for the attention blocks' Linears (K = 64, N in {64, 192}, the
 * split-bf16 and bf16 matrix modes): ONE launch reads gy [rows, N] and x [rows, K] once and writes
 * gx[rows,K] = gy W (bitwise spt_skinny_linear_wt_m_f32's), gw[N,K] = gy^T x_n and gb[N] (nullable)
 * = column sums of gy; x_n = x through the pre-norm tables of spt_skinny_dw_pre_m_f32 (pre_am NULL
 * = plain x; the instance given the tables is bitwise the plain one given the normalised rows).
 * One [N x K | N] table per workgroup, summed in a fixed order (deterministic).
 * ws: spt_skinny_linear_bwd_workspace_bytes(K, N) bytes of device scratch, checked before any launch.
 * spt_skinny_bwd_fused: process switch the autograd wrappers consult (default on; the environment's
 * SPT_SKINNY_BWD_FUSED=0 turns it off; < 0: query); returns the previous value. */
int spt_skinny_linear_bwd_supported(int K, int N, int num_graphs, int mode);
size_t spt_skinny_linear_bwd_workspace_bytes(int K, int N);
int spt_skinny_linear_bwd_m_f32(const float* gy, const float* x, const float* W, int64_t rows, int N,
                                int K, float* gx, float* gw, float* gb, const float* pre_am,
                                const float* pre_scale, const float* pre_bias, const int64_t* batch,
                                int num_graphs, int mode, void* ws, size_t ws_bytes,
                                spt_stream_t stream);
int spt_skinny_bwd_fused(int on);
/* Narrow Linears (N <= 16 outputs: the classifier heads, src/nn/mlp.py:128-142).  Forward: the
 * skinny kernel above accepts N <= 16 with K in {32, 64, 128} (missing columns read as zero, not
 * stored).  Backward in ONE pass over x and gy for K = 64 and (round 5: the KITTI-360 width's heads,
 * two 64-column slabs) K = 128: gx[rows,K] = gy W (nullable),
 * gw[N,K] = gy^T x, gb[N] = column sums of gy (nullable); per-wave partials, fixed-order sum. */
int spt_narrow_linear_bwd_supported(int K, int N);
size_t spt_narrow_linear_bwd_workspace_bytes(int K, int N);
int spt_narrow_linear_bwd_f32(const float* gy, const float* x, const float* W, int64_t rows, int N,
                              int K, float* gx, float* gw, float* gb, void* ws, size_t ws_bytes,
                              spt_stream_t stream);

/* Pieces of the GraphNorm two-pass scheme for callers that produce / consume the
 * per-graph totals themselves (the fused MLP layers below).  totals layout:
 * [num_graphs][2d+1] f64 = (column sums, column sums of the second quantity, row count). */
int spt_graphnorm_tables_f32(const double* total, int num_graphs, int d, const float* weight,
                             const float* mean_scale, float eps, float* mean, float* rstd,
                             float* am, float* scale, spt_stream_t stream);
int spt_graphnorm_apply_f32(const float* x, const int64_t* batch, int64_t r, int d,
                            int num_graphs, const float* am, const float* scale,
                            const float* bias, float act_slope, float* y, spt_stream_t stream);
int spt_graphnorm_bwd_stats_f32(const float* x, const float* gy, const int64_t* batch, int64_t r,
                                int d, int num_graphs, const float* am, const float* scale,
                                const float* bias, float act_slope, double* total, void* ws,
                                size_t ws_bytes, spt_stream_t stream);
/* The totals of spt_graphnorm_bwd_stats_f32 when gy is the backward of a segment max-pool
 * (one non-zero per (segment, channel): gy[arg[s,c], c] = gout[s,c]), computed from
 * (gout, arg [num_seg, d], the raw rows x gathered at arg) without a pass over [r, d] tensors.
 * seg_graph [num_seg] (NULL = one graph), graph_rows [B] int64 = rows of every graph. */
size_t spt_graphnorm_bwd_stats_sparse_workspace_bytes(int64_t num_seg, int d, int num_graphs);
int spt_graphnorm_bwd_stats_sparse_f32(const float* x, const float* gout, const int32_t* arg,
                                       const int64_t* seg_graph, const int64_t* graph_rows,
                                       int64_t num_seg, int64_t n, int d, int num_graphs,
                                       const float* am, const float* scale, const float* bias,
                                       float act_slope, double* total, void* ws,
                                       size_t ws_bytes, spt_stream_t stream);
/* x_is_bf16 = 1: x holds bf16 values (SPT_FMLP_H_BF16 below); 2: x is raw [num_seg, d] f32. */
int spt_graphnorm_bwd_stats_sparse_ex_f32(
    const void* x, int x_is_bf16, const float* gout, const int32_t* arg, const int64_t* seg_graph,
    const int64_t* graph_rows, int64_t num_seg, int64_t n, int d, int num_graphs,
    const float* am, const float* scale, const float* bias, float act_slope, double* total,
    void* ws, size_t ws_bytes, spt_stream_t stream);
/* The same totals from raw [num_seg, d] = the layer output at the arg rows as the pool wrote it
 * (spt_segcsr_max_affine_raw_f32): a stream, no gather.  n = rows of the layer (arg's sentinel). */
int spt_graphnorm_bwd_stats_sparse_raw_f32(
    const float* raw, const float* gout, const int32_t* arg, const int64_t* seg_graph,
    const int64_t* graph_rows, int64_t num_seg, int64_t n, int d, int num_graphs,
    const float* am, const float* scale, const float* bias, float act_slope, double* total,
    void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_graphnorm_bwd_tables_f32(const double* total, int num_graphs, int d, const float* weight,
                                 const float* mean_scale, const float* mean, const float* rstd,
                                 float* c1, float* c2, float* c3, float* gweight, float* gbias,
                                 float* gmean_scale, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused MLP layer: bias-free Linear whose input is the previous layer's RAW output
 * (GraphNorm-apply + LeakyReLU happen while the tile is staged) and whose epilogue
 * yields the statistics of its own GraphNorm.  Replaces, per layer of
 * src/nn/mlp.py:8-94, one library GEMM + GraphNorm statistics pass + GraphNorm apply
 * pass (forward), and GraphNorm backward apply + the dX / dW GEMMs (backward).
 * One call covers the rows [r0, r1) of ONE graph of the batch.
 *   x / xprev [rows, K] raw, W [N, K], h [rows, N] raw output; pre_* = (am, scale
 *   [K], bias [K], slope) of the previous GraphNorm or NULL (layer input used as is);
 *   total [2N+1] f64 out; backward: gy, h [rows, N], this layer's (am, scale, bias,
 *   slope) and backward rows (c1, c2, c3); gx [rows, K] or NULL; gW [N, K] (+= when
 *   accumulate); prev_total [2K+1] = statistics for the previous GraphNorm's backward.
 * ---------------------------------------------------------------------- */
int spt_fused_linear_supported(int K, int N);
/* Matrix pipe of the fused layers' GEMMs.  0: f32 in / f32 accumulate everywhere (bitwise an
 * fmaf chain).  1 (default): the backward GEMMs (gW, gx) on the bf16 pipe with split operands
 * (each f32 product = hi*hi + lo*hi + hi*lo of bf16 halves, f32 accumulate, ~2^-17 relative per product: 17 of f32's 24 bits -
 * a tenth of the gradients' parity bar); the forward stays exact f32 (its outputs feed
 * GraphNorm statistics, bar 2e-5).  2: forward too.  Returns the previous setting. */
int spt_fused_linear_use_split_bf16(int mode);
size_t spt_fused_linear_workspace_bytes(int K, int N);
int spt_fused_linear_fwd_f32(const float* x, int64_t r0, int64_t r1, int K, const float* W,
                             int N, const float* pre_am, const float* pre_scale,
                             const float* pre_bias, float pre_slope, float* h, double* total,
                             void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_fused_linear_bwd_f32(const float* gy, const float* h, int64_t r0, int64_t r1, int N,
                             const float* am, const float* scale, const float* bias,
                             float slope, const float* c1, const float* c2, const float* c3,
                             const float* xprev, int K, const float* pre_am,
                             const float* pre_scale, const float* pre_bias, float pre_slope,
                             const float* W, float* gx, float* gW, int accumulate,
                             double* prev_total, void* ws, size_t ws_bytes, spt_stream_t stream);
/* Backward of the TOP layer of a fused MLP whose output went through a segment max-pool
 * (MaxPool(MLP(x)), nn/stage.py:429-431): the pool's gradient (gout [S,N], arg [S,N]) is consumed
 * directly - rows are visited in the pool's CSR order (positions [p0, p1) of perm; pos_seg[j] =
 * segment of position j), h / xprev rows gathered, gx rows scattered - so the dense [rows, N]
 * gradient the pool's backward would write (and this layer read back) never exists.  Other
 * arguments as spt_fused_linear_bwd_f32.  spt_fused_linear_pooled_supported: built shapes, under
 * the current matrix mode (split-bf16 kernels only). */
int spt_fused_linear_pooled_supported(int K, int N);
/* Per-call matrix mode (no process-wide state): the *_ex entries take `mode` = 0..3 as
 * spt_fused_linear_use_split_bf16 describes them (< 0: the process default), so that two models
 * at different precisions, or two streams, never change each other's arithmetic. */
int spt_fused_linear_pooled_supported_ex(int K, int N, int mode);
/* Tile staging of the split-bf16 / bf16 backward kernels: LDS-DMA (global_load_lds: one memory
 * round trip per 16-row tile, csrc/fused_mlp_dma.hip; default, where the (K, N) is built: 64->128,
 * 64->64, 32->64, and 32->32 for dense f32 rows) or register-staged (csrc/fused_mlp.hip).  Same arithmetic, same summation order
 * inside a tile.  Process-wide: spt_fused_linear_bwd_use_dma(0 | 1) (< 0: query), returns the
 * previous setting; per call: OR SPT_FMLP_BWD_REGISTER_STAGED into the `mode` of the *_ex entries. */
#define SPT_FMLP_BWD_REGISTER_STAGED 4
/* bf16 ACTIVATION STORAGE (the reference's `precision: bf16`, configs/trainer/gpu.yaml:7-10: under
 * autocast the Linear outputs ARE bf16 tensors).  With matrix mode 3 in the mode word of the *_ex /
 * *_runs entries: SPT_FMLP_H_BF16 = the layer's raw output h is written (forward) / read (backward)
 * as bf16 [rows, N]; SPT_FMLP_X_BF16 = the layer's input x / xprev holds bf16 values (the previous
 * layer's h).  Statistics, gradients and tables stay f32 / f64.  spt_fused_linear_storage_supported:
 * shapes built with this option (the point MLP's). */
#define SPT_FMLP_H_BF16 8
#define SPT_FMLP_X_BF16 16
int spt_fused_linear_storage_supported(int K, int N);
int spt_fused_linear_bwd_use_dma(int on);
/* The staging the dense backward with gx of K -> N (K0 == 0), or the fold of K0 -> K under K -> N
 * (K0 > 0, see spt_fused_linear_bwd_fold_supported), takes under `mode` and the process-wide switch:
 * 1 = LDS-DMA, 0 = register-staged, -1 = the fold is not built.  The two stagings give the same
 * bits, so this is how a caller or a test tells them apart. */
int spt_fused_linear_bwd_route(int K0, int K, int N, int mode);
/* Forward of matrix mode 1 (the default "f32"): 1 (default) = the f32 product as SIX bf16 products
 * of 3-way split operands on the bf16 matrix pipe (f32-exact: every dropped term is below 2^-24 of
 * its product), 0 = the f32 matrix pipe.  Process-wide; < 0 queries; returns the previous setting. */
int spt_fused_linear_fwd_use_x3(int on);
int spt_fused_linear_fwd_ex_f32(const float* x, int64_t r0, int64_t r1, int K, const float* W,
                                int N, const float* pre_am, const float* pre_scale,
                                const float* pre_bias, float pre_slope, float* h, double* total,
                                int mode, void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_fused_linear_bwd_ex_f32(const float* gy, const float* h, int64_t r0, int64_t r1, int N,
                                const float* am, const float* scale, const float* bias,
                                float slope, const float* c1, const float* c2, const float* c3,
                                const float* xprev, int K, const float* pre_am,
                                const float* pre_scale, const float* pre_bias, float pre_slope,
                                const float* W, float* gx, float* gW, int accumulate,
                                double* prev_total, int mode, void* ws, size_t ws_bytes,
                                spt_stream_t stream);
int spt_fused_linear_bwd_pooled_ex_f32(
    const float* gout, const int32_t* arg, const int32_t* perm, const int32_t* pos_seg,
    const float* h, int64_t p0, int64_t p1, int N, const float* am, const float* scale,
    const float* bias, float slope, const float* c1, const float* c2, const float* c3,
    const float* xprev, int K, const float* pre_am, const float* pre_scale, const float* pre_bias,
    float pre_slope, const float* W, float* gx, float* gW, int accumulate, double* prev_total,
    int mode, void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_fused_linear_bwd_pooled_f32(
    const float* gout, const int32_t* arg, const int32_t* perm, const int32_t* pos_seg,
    const float* h, int64_t p0, int64_t p1, int N, const float* am, const float* scale,
    const float* bias, float slope, const float* c1, const float* c2, const float* c3,
    const float* xprev, int K, const float* pre_am, const float* pre_scale, const float* pre_bias,
    float pre_slope, const float* W, float* gx, float* gW, int accumulate, double* prev_total,
    void* ws, size_t ws_bytes, spt_stream_t stream);

/* The rows of SEVERAL graphs in ONE launch of the fused layer kernels (a batch of B clouds, or an
 * index that is sorted only piecewise - the edge MLP's norm index norm_index[edge_index[0]],
 * src/models/components/spt.py:829-836, is sorted inside each third of [i<j | j>i | loops]).
 * Run r covers rows [run_r0[r], run_r1[r]) of graph run_graph[r]; HOST arrays, 1 <= nruns <= 16,
 * sorted by graph, num_graphs <= 16.  Per-graph tables are [num_graphs, width] arrays, `total` /
 * `prev_total` [num_graphs, 2 width + 1] (a graph without rows reads as zeros), gW = the sum over
 * all runs.  Otherwise as the one-range entries above. */
int spt_fused_linear_fwd_runs_f32(const float* x, int nruns, const int64_t* run_r0,
                                  const int64_t* run_r1, const int32_t* run_graph, int num_graphs,
                                  int K, const float* W, int N, const float* pre_am,
                                  const float* pre_scale, const float* pre_bias, float pre_slope,
                                  float* h, double* total, int mode, void* ws, size_t ws_bytes,
                                  spt_stream_t stream);
int spt_fused_linear_bwd_runs_f32(
    const float* gy, const float* h, int nruns, const int64_t* run_r0, const int64_t* run_r1,
    const int32_t* run_graph, int num_graphs, int N, const float* am, const float* scale,
    const float* bias, float slope, const float* c1, const float* c2, const float* c3,
    const float* xprev, int K, const float* pre_am, const float* pre_scale, const float* pre_bias,
    float pre_slope, const float* W, float* gx, float* gW, double* prev_total, int mode, void* ws,
    size_t ws_bytes, spt_stream_t stream);
int spt_fused_linear_bwd_pooled_runs_f32(
    const float* gout, const int32_t* arg, const int32_t* perm, const int32_t* pos_seg,
    const float* h, int nruns, const int64_t* run_p0, const int64_t* run_p1,
    const int32_t* run_graph, int num_graphs, int N, const float* am, const float* scale,
    const float* bias, float slope, const float* c1, const float* c2, const float* c3,
    const float* xprev, int K, const float* pre_am, const float* pre_scale, const float* pre_bias,
    float pre_slope, const float* W, float* gx, float* gW, double* prev_total, int mode, void* ws,
    size_t ws_bytes, spt_stream_t stream);
/* Round 6: the same three calls with a GraphNorm descriptor - the layer's own norm (forward: its
 * tables mean / rstd / am / scale come out of the call, spt_graphnorm_tables_f32 is not needed;
 * `total` may be NULL) or the PREVIOUS layer's norm (backward: its c1 / c2 / c3 and parameter
 * gradients come out of the call, spt_graphnorm_bwd_tables_f32 is not needed; `prev_total` may be
 * NULL).  One "post" launch per call sums the partial tables and writes the norm's tables: a fused
 * layer costs 2 launches per direction instead of 3 (forward) / 4 (backward) - what a train-batch
 * step, ~360 launches of a few microseconds, is made of. */
int spt_fused_linear_fwd_runs_gn_f32(const float* x, int nruns, const int64_t* run_r0,
                                     const int64_t* run_r1, const int32_t* run_graph, int num_graphs,
                                     int K, const float* W, int N, const float* pre_am,
                                     const float* pre_scale, const float* pre_bias, float pre_slope,
                                     float* h, double* total, int mode, void* ws, size_t ws_bytes,
                                     const spt_gn_fwd_tables* norm, spt_stream_t stream);
int spt_fused_linear_bwd_runs_gn_f32(
    const float* gy, const float* h, int nruns, const int64_t* run_r0, const int64_t* run_r1,
    const int32_t* run_graph, int num_graphs, int N, const float* am, const float* scale,
    const float* bias, float slope, const float* c1, const float* c2, const float* c3,
    const float* xprev, int K, const float* pre_am, const float* pre_scale, const float* pre_bias,
    float pre_slope, const float* W, float* gx, float* gW, double* prev_total, int mode, void* ws,
    size_t ws_bytes, const spt_gn_bwd_tables* prev_norm, spt_stream_t stream);
/* The chain's BOTTOM layer K0 -> K folded into the backward of the layer K -> N above it: the bottom
 * layer is bias-free and its input x0 [rows, K0] (raw f32, no norm in front; 16-byte aligned where
 * K0 % 4 == 0, else 4-byte) needs
 * no gradient, so all its backward produces is gW0 [K, K0].  This call takes the sums gW0 is made
 * of inside the upper layer's kernel, stores no gx and writes gW0 from its post launch (together
 * with the bottom norm's tables in prev_norm, which is required; W0 [K, K0] = the bottom weight).
 * _supported: 1 when the shape pair is built for the matrix mode - 12 -> 32 under 32 -> 64 (DMA-staged
 * backward) and 18 -> 32 under 32 -> 32 (DMA-staged or register-staged), in the default f32 mode (f32-exact split forward, split-bf16
 * backward; no bf16 storage). */
int spt_fused_linear_bwd_fold_supported(int K0, int K, int N, int mode);
int spt_fused_linear_bwd_runs_gn_fold_f32(
    const float* gy, const float* h, int nruns, const int64_t* run_r0, const int64_t* run_r1,
    const int32_t* run_graph, int num_graphs, int N, const float* am, const float* scale,
    const float* bias, float slope, const float* c1, const float* c2, const float* c3,
    const float* xprev, int K, const float* pre_am, const float* pre_scale, const float* pre_bias,
    float pre_slope, const float* W, float* gW, int mode, void* ws, size_t ws_bytes,
    const spt_gn_bwd_tables* prev_norm, const float* x0, int K0, const float* W0, float* gW0,
    spt_stream_t stream);
int spt_fused_linear_bwd_pooled_runs_gn_f32(
    const float* gout, const int32_t* arg, const int32_t* perm, const int32_t* pos_seg,
    const float* h, int nruns, const int64_t* run_p0, const int64_t* run_p1,
    const int32_t* run_graph, int num_graphs, int N, const float* am, const float* scale,
    const float* bias, float slope, const float* c1, const float* c2, const float* c3,
    const float* xprev, int K, const float* pre_am, const float* pre_scale, const float* pre_bias,
    float pre_slope, const float* W, float* gx, float* gW, double* prev_total, int mode, void* ws,
    size_t ws_bytes, const spt_gn_bwd_tables* prev_norm, spt_stream_t stream);

/* Consistency check of a stored segment CSR (pointers [num_seg + 1], points [n], int64 as the
 * reference's Cluster keeps them, src/data/cluster.py:19-77) against the index it is to be adopted
 * as the view of (idx [n] int64): ORs into *flag (int32, device; the caller clears it) bit 0 =
 * pointers not 0 .. n / decreasing, bit 1 = a point outside [0, n), bit 2 = idx[points[j]] is not
 * the segment holding position j, bit 3 (check_ascending) = a segment's points not ascending.
 * One launch, no host round trip. */
int spt_csr_check_i64(const int64_t* idx, const int64_t* points, const int64_t* pointers, int64_t n,
                      int64_t num_seg, int check_ascending, int32_t* flag, spt_stream_t stream);
/* Round 6: the same check AND the int32 view the segment kernels read, in one launch - what
 * csr.adopt_csr runs when it installs nag[i+1].sub as the view of nag[i].super_index
 * (src/data/cluster.py:19-77, src/data/nag.py:306-399).  perm32 [n] = points clamped into [0, n),
 * rowptr32 [num_seg + 1] = pointers clamped into [0, n]: a stored CSR that fails the check cannot
 * lead a segment kernel outside its buffers before the (deferred) verdict has been read.  The
 * ascending comparison (bit 3) always runs.  *flag as above (the caller clears it). */
int spt_csr_adopt_i64(const int64_t* idx, const int64_t* points, const int64_t* pointers, int64_t n,
                      int64_t num_seg, int32_t* perm32, int32_t* rowptr32, int32_t* flag,
                      spt_stream_t stream);

/* ------------------------------------------------------------------------
 * The point MLP's TOP layer and the max-pool behind it as one unit     (a1 + a2 + a5, round 5)
 * Replaces, for the layer whose output feeds only the level-0 -> level-1 max-pool
 * (src/nn/stage.py:413-431: PointStage MLP -> pool; layer = bias-free Linear -> GraphNorm ->
 * LeakyReLU, src/nn/mlp.py:43-56; pool = MaxPool, src/nn/pool.py:61-82), the sequence
 * spt_fused_linear_fwd_* -> spt_graphnorm_tables_f32 -> spt_segcsr_max_affine_* (forward) and
 * spt_fused_linear_bwd_pooled_* (backward): the layer's [rows, N] output is never written, read
 * or recomputed (csrc/fused_pool.hip explains the three identities used).
 *   forward : out [num_seg, N] = max over the segment's rows of leaky(GraphNorm(x_act W^T)), bitwise
 *             the value of norm-then-pool evaluated with THESE statistics; arg [num_seg, N] int32 =
 *             first row attaining the raw extremum (n_rows for an empty segment, like
 *             spt_segcsr_reduce_f32; the reference's arg except on ties of y between rows of
 *             different h); argpos [num_seg, N] int32 = the CSR position of that row (arg =
 *             perm[argpos]: what the backward scatters by; arg may be NULL (round 6): a caller that only
 *             runs the fused backward needs the positions alone, and the row ids cost one scattered
 *             4-byte read per (segment, channel)); raw [num_seg, N] = h of the arg row; gram [num_graphs, K K + K + 1] f64
 *             = (sum_i y_i y_i^T | sum_i y_i | rows) of the layer's activated INPUT per graph, from
 *             which the norm's statistics are evaluated (total [num_graphs, 2N+1], nullable, receives
 *             them in spt_fused_linear_fwd_*'s layout) and its tables mean / rstd / am / scale
 *             [num_graphs, N] are written (spt_graphnorm_tables_f32's formulas).
 *             x [n_rows, K]: RAW output of the previous layer (f32, or bf16 with SPT_FMLP_X_BF16 in
 *             `mode`), pre_* its norm tables ([num_graphs, K], [num_graphs, K], [K]) and slope;
 *             (perm, pos_seg, rowptr): the pool's CSR view and the segment of every CSR position;
 *             runs: the graphs' CSR position ranges (contiguous, tiling [0, n_rows)); seg_graph
 *             [num_seg] int64 (NULL with one graph).
 *   backward: from gout, raw, argpos [num_seg, N] and the GraphNorm-backward coefficient rows c1 / c2 / c3
 *             (spt_graphnorm_bwd_stats_sparse_raw_f32 -> spt_graphnorm_bwd_tables_f32) to gx
 *             [n_rows, K] (gradient of the previous layer's normalised output), gW [N, K] and
 *             prev_total [num_graphs, 2K+1] (statistics of the previous norm's backward);
 *             gm [num_seg, N] f32: scratch of the call.
 *   mode    : the fused layers' mode word; built for matrix modes 1 (f32-exact 3-way split forward),
 *             2 and 3, K in {32, 64}, N in {64, 128} (spt_fused_linear_pool_supported).
 *   ws      : spt_fused_linear_pool_workspace_bytes(K, N). */
int spt_fused_linear_pool_supported(int K, int N, int mode);
size_t spt_fused_linear_pool_gram_len(int K);
size_t spt_fused_linear_pool_workspace_bytes(int K, int N);
int spt_fused_linear_fwd_pool_runs_f32(
    const void* x, const int32_t* perm, const int32_t* pos_seg, const int32_t* rowptr,
    const int64_t* seg_graph, int64_t num_seg, int64_t n_rows, int nruns, const int64_t* run_p0,
    const int64_t* run_p1, const int32_t* run_graph, int num_graphs, int K, const float* W, int N,
    const float* gn_weight, const float* gn_bias, const float* gn_mean_scale, float eps, float slope,
    const float* pre_am, const float* pre_scale, const float* pre_bias, float pre_slope, float* out,
    int32_t* arg, int32_t* argpos, float* raw, double* gram, double* total, float* mean, float* rstd,
    float* am, float* scale, int mode, void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_fused_linear_bwd_pool_runs_f32(
    const float* gout, const float* raw, const int32_t* argpos, const int32_t* perm,
    const int32_t* pos_seg, const int64_t* seg_graph, int64_t num_seg, int nruns,
    const int64_t* run_p0, const int64_t* run_p1, const int32_t* run_graph, int num_graphs, int N,
    const float* am, const float* scale, const float* bias, float slope, const float* c1,
    const float* c2, const float* c3, const void* xprev, int K, const float* pre_am,
    const float* pre_scale, const float* pre_bias, float pre_slope, const float* W,
    const double* gram, float* gm, float* gx, float* gW, double* prev_total, int mode, void* ws,
    size_t ws_bytes, spt_stream_t stream);
/* ... with the previous layer's GraphNorm-backward tables written by the call (round 6, see
 * spt_fused_linear_bwd_runs_gn_f32; prev_total may be NULL). */
int spt_fused_linear_bwd_pool_runs_gn_f32(
    const float* gout, const float* raw, const int32_t* argpos, const int32_t* perm,
    const int32_t* pos_seg, const int64_t* seg_graph, int64_t num_seg, int nruns,
    const int64_t* run_p0, const int64_t* run_p1, const int32_t* run_graph, int num_graphs, int N,
    const float* am, const float* scale, const float* bias, float slope, const float* c1,
    const float* c2, const float* c3, const void* xprev, int K, const float* pre_am,
    const float* pre_scale, const float* pre_bias, float pre_slope, const float* W,
    const double* gram, float* gm, float* gx, float* gW, double* prev_total, int mode, void* ws,
    size_t ws_bytes, const spt_gn_bwd_tables* prev_norm, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Cross-entropy of the classifier heads' logits                (train step)
 * torch.nn.CrossEntropyLoss(ignore_index=...) of configs/model/semantic/default.yaml:47-49 as
 * src/models/semantic.py applies it per output level: mean over the rows whose target is not
 * ignore_index of logsumexp(logits[row]) - logits[row, target[row]].  C <= 32 classes.
 *   fwd: lse[rows] (kept for the backward), loss[1], count[1] (rows that counted, as f32);
 *        ws: spt_cross_entropy_workspace_bytes(rows).  Deterministic (f64 partial sums, fixed order).
 *        A target outside [0, C) other than ignore_index makes the loss NaN (torch: device assert).
 *   bwd: glogits = (softmax - onehot) * gout[0] / count[0]; gout / count are device scalars. */
size_t spt_cross_entropy_workspace_bytes(int64_t rows);
int spt_cross_entropy_fwd_f32(const float* logits, const int64_t* target, int64_t rows, int C,
                              int64_t ignore_index, float* lse, float* loss, float* count,
                              void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_cross_entropy_bwd_f32(const float* logits, const int64_t* target, const float* lse,
                              int64_t rows, int C, int64_t ignore_index, const float* gout,
                              const float* count, float* glogits, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * The default semantic criterion: class weights, label-histogram targets   (train / val step)
 * configs/model/semantic/default.yaml:7-12 (loss_type 'ce_kl', weighted_loss True) as
 * src/models/semantic.py:397-474 builds it from CrossEntropyLoss(weight, ignore_index = C) and
 * loss_with_target_histogram (src/utils/loss.py:25-38), with no [nnz, C] expansion and no host
 * round trip.  logits f32 [rows, C <= 32]; weight f32 [C] or NULL (ones); mode:
 *   0 index:     target int64 [rows]; rows with target == ignore_index do not count
 *                loss = sum w[t] (lse - z[t]) / sum w[t]
 *   1 dominant:  target int64 [rows, ncols] label counts, ncols in {C, C + 1} (column C = void);
 *                t = first index of the row maximum over all ncols columns, t == C is ignored;
 *                the formula of mode 0
 *   2 histogram: loss = sum_r sum_{c < C} h[r, c] w[c] (lse_r - z[r, c]) / sum_r sum_{c < ncols} h[r, c]
 *                (the void column counts in the denominator only; class weights do not enter it)
 *   fwd: loss[1] f32, den[1] f64 (the denominator; exact for counts below 2^53);
 *        ws: spt_cross_entropy_workspace_bytes(rows).  Deterministic (f64 partial sums, fixed order).
 *        A label outside [0, C) other than ignore_index, or a negative count, makes the loss NaN;
 *        den == 0 (every row ignored / empty) gives NaN like the reference's 0 / 0.
 *        confmat (modes 1 / 2; may be NULL): int64 [C, C], confmat[t, argmax z[r]] += h[r, t] for
 *        t < C (first maximum), ADDED to what the caller's buffer holds (integer atomics: exact in
 *        any order).
 *   bwd: glogits[r, c] = gout[0] (S_r softmax(z[r])[c] - hw[r, c]) / den[0], with hw = h w and
 *        S_r = sum_{c < C} hw[r, c] (mode 2), hw = w[t] onehot(t) and S_r = w[t] (modes 0 / 1; 0
 *        for ignored rows).  gout / den are device scalars.  The softmax is recomputed from the
 *        logits and the difference formed in f64. */
int spt_hist_loss_fwd_f32(const float* logits, const int64_t* target, int64_t rows, int C, int ncols,
                          int mode, int64_t ignore_index, const float* weight, float* loss,
                          double* den, int64_t* confmat, void* ws, size_t ws_bytes,
                          spt_stream_t stream);
int spt_hist_loss_bwd_f32(const float* logits, const int64_t* target, int64_t rows, int C, int ncols,
                          int mode, int64_t ignore_index, const float* weight, const float* gout,
                          const double* den, float* glogits, spt_stream_t stream);
/* Edge-affinity loss of the panoptic model (PanopticSegmentationModule.model_step,
 * src/models/panoptic.py:726-796): BCE with logits of logits f32 [E] against target f32 [E] over
 * the edges (i, j) = edge_index int64 [2, E] with keep = !(node_void[i] && node_void[j]); nothing
 * is compacted.  Per kept edge: kind = 2 (node_y[i] != node_y[j]) + (node_obj[i] != node_obj[j]),
 * w = case_weight[kind] (f32 [4]; NULL: 1), pw = pos_weight[0] (a DEVICE scalar; NULL: 1),
 *   l = (1 - t) x + (1 + (pw - 1) t) (max(-x, 0) + log1p(exp(-|x|)))      evaluated in f64.
 *   fwd: loss[1] f32 = sum w l / sum w, den[1] f64 = sum w (without a table: the number of kept
 *        edges, the loss their mean).  No kept edge: 0 / 0 = NaN.  f64 partial sums per workgroup
 *        added in a fixed order: bitwise reproducible.  ws: spt_edge_affinity_loss_workspace_bytes.
 *        stats (may be NULL) int64 [4] += tp, fp, tn, fn of (x > 0) against (t > 0.5) over the
 *        kept edges.  status (may be NULL) int32 [1] += edges with an end outside [0, N): dropped.
 *   bwd: glogits[e] = gout[0] w / den[0] ((1 + (pw - 1) t) sigmoid(x) - pw t) for a kept edge
 *        (= (1 - t) - (1 + (pw - 1) t) sigmoid(-x), in the form torch's backward evaluates),
 *        an explicit 0 for a dropped one.  gout / den are device scalars. */
size_t spt_edge_affinity_loss_workspace_bytes(int64_t E);
int spt_edge_affinity_loss_fwd_f32(const float* logits, const float* target,
                                   const int64_t* edge_index, int64_t E, const uint8_t* node_void,
                                   const int64_t* node_obj, const int64_t* node_y, int64_t N,
                                   const float* case_weight, const float* pos_weight, float* loss,
                                   double* den, int64_t* stats, int32_t* status, void* ws,
                                   size_t ws_bytes, spt_stream_t stream);
int spt_edge_affinity_loss_bwd_f32(const float* logits, const float* target,
                                   const int64_t* edge_index, int64_t E, const uint8_t* node_void,
                                   const int64_t* node_obj, const int64_t* node_y, int64_t N,
                                   const float* case_weight, const float* pos_weight,
                                   const float* gout, const double* den, float* glogits,
                                   spt_stream_t stream);
/* Edge-contrast focal loss of the partition training stage (PartitionCriterion with
 * BinaryFocalLoss, src/loss/partition_criterion.py:92-145, src/loss/focal.py:194-220), without
 * compacting the edge list and without a host read.  x f32 [N, D] (row stride ldx elements,
 * 1 <= D <= 128), y int64 label histograms [N, ycols >= C] (columns past C are void) or, with
 * ycols == 0, int64 labels [N] (outside [0, C): void), edge_index int64 [2, E] in any order.
 *   label_n = first arg-max of y[n, :C]; a node is void when that maximum is 0.
 *   An edge (i, j) is dropped if i == j or an end is void; an end outside [0, N) drops it too and
 *   is counted.  Otherwise t = (label_i == label_j): inter (t = 0) or intra (t = 1).
 *   ratio < 0: every kept edge is selected.  ratio in (0, 1]: all inter edges and exactly
 *   n_major = (int) (f32(n_inter) * f32(1 / ratio - 1)) intra edges (clamped to n_intra), those
 *   with the smallest keys (rand32(s, e) << 32 | e), e the position in the list, s = seed ^
 *   (rand32(0x5EED, 2 calls) << 32 | rand32(0x5EED, 2 calls + 1)) with (seed, calls) = state[0..1]
 *   (a DEVICE int64 [2]); the last kernel adds 1 to state[1].
 *   Per selected edge, in f64: d = |x_i - x_j|, p = exp(-d / T), q = t ? p : 1 - p,
 *   q' = eps + (1 - 2 eps) q, w = t ? weight : 1 - weight, l = -w (1 - q')^gamma log q'.
 *   fwd: loss[1] f32 = sum l / n_selected (f64 partial sums per workgroup, added in a fixed
 *        order), exactly 0 when nothing is selected or there is no inter edge; den[1] f64 =
 *        n_selected, 0 in that case (the backward's switch).  code uint8 [E] out: 0 not selected,
 *        1 inter, 2 intra - the backward's input.  counts (may be NULL) int64 [3] = n_inter,
 *        n_intra, n_selected (written).  status (may be NULL) int32 [2]: [0] += edges with an end
 *        out of range, [1] |= 1 when n_major was clamped.  selected (may be NULL) uint8 [E] = the
 *        selection as 0 / 1.  ws: spt_partition_loss_workspace_bytes.
 *   bwd: gx[n] = gout[0] / den[0] * sum over the selected edges e at n of c_e (x_n - x_other(e)),
 *        c_e = dl/dd / d (0 at d == 0); one lane group per node walks its run of the by-source
 *        view, then of the by-target view (spt_csr_build of the two rows of edge_index with ends
 *        clamped into [0, N)), and writes the row once: no atomics, zero rows for isolated nodes
 *        and when den[0] == 0.  gout / den are device scalars. */
size_t spt_partition_loss_workspace_bytes(int64_t N, int64_t E);
int spt_partition_loss_fwd_f32(const float* x, int64_t ldx, int64_t N, int D, const int64_t* y,
                               int ycols, int C, const int64_t* edge_index, int64_t E,
                               double temperature, double gamma, double weight, double epsilon,
                               double ratio, int64_t* state, float* loss, double* den, uint8_t* code,
                               int64_t* counts, int32_t* status, uint8_t* selected, void* ws,
                               size_t ws_bytes, spt_stream_t stream);
int spt_partition_loss_bwd_f32(const float* x, int64_t ldx, int64_t N, int D,
                               const int64_t* edge_index, int64_t E, const uint8_t* code,
                               const int32_t* src_rowptr, const int32_t* src_perm,
                               const int32_t* tgt_rowptr, const int32_t* tgt_perm,
                               double temperature, double gamma, double weight, double epsilon,
                               const float* gout, const double* den, float* gx, int64_t ldg,
                               spt_stream_t stream);
/* Confusion matrix from segment-level predictions and label histograms, without flattening them
 * to points (ConfusionMatrix.update, src/metrics/semantic.py:66-107): confmat[t, pred[r]] +=
 * h[r, t] for t < C <= 32 (target int64 [rows, ncols >= C]; columns past C are void), or, with
 * ncols == 0, confmat[target[r], pred[r]] += 1 for int64 labels in [0, C) (any other label is
 * void).  int64 [C, C], ADDED to what the buffer holds; rows whose prediction is not in [0, C) are
 * dropped. */
int spt_confusion_matrix_i64(const int64_t* pred, const int64_t* target, int64_t rows, int C,
                             int ncols, int64_t* confmat, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Augmentations of the per-batch training chain              (csrc/augment.hip)
 * NAGJitterKey, NAGDropoutColumns, NAGDropoutRows (src/transforms/data.py:440-721),
 * RandomTiltAndRotate, RandomAnisotropicScale, RandomAxisFlip (src/transforms/geometry.py:
 * 28-245), NAGColorAutoContrast, NAGColorDrop (src/transforms/point.py:374-545).
 *
 * Every entry: f32; element (i, c) of a tensor at p[i * ld + c] (ld = column count for a tensor
 * of its own, ld = F and p = x + column for a block of a wider [n, F] table); out may equal the
 * input; n = 0 returns 0 without a launch; no host read.  The values depend on (seed, logical
 * index) only, never on ld, alignment or grid size.
 *
 * Random stream: r = rand32(seed, counter), the splitmix64 finaliser of the sampler, with the
 * counter of an element its logical index i * n_cols + c and the counter of a row decision i.
 *   decision: u = (r >> 8) * 2^-24 in [0, 1), taken when u < p (f32 compare).
 *   noise:    u = ((r >> 8) + 0.5) * 2^-24 in (0, 1),
 *             clamp(sigma * sqrt(2) * erfinv(lo + u * (hi - lo)), -trunc, trunc)
 *             with lo = 2 Phi(-trunc / sigma) - 1 and hi = 2 Phi(trunc / sigma) - 1 from the
 *             caller (torch.nn.init.trunc_normal_); trunc <= 0: lo = -1, hi = 1 and no clamp
 *             (the tail then ends at 5.42 sigma).  Always finite.
 *
 * spt_augment_features_f32: flags bit 0 x += noise(seed_jitter), bit 1 zero the columns whose
 *   bit is set in col_mask (n_cols <= 64), bit 2 zero the rows with u(seed_rows, i) < p_rows,
 *   in this order.
 * spt_augment_geometry_f32: mode 0 pos [n, 3], 1 normal [n, 3], 2 edge_attr [n, 7].  flags bit 0
 *   jitter (pos only), bit 1 rotate v <- v R^T (rotation: 9 HOST floats, row major), bit 2
 *   scale (scale: 3 HOST floats; normal: then v / max(||v||, 1e-12); edge: columns 3..6 times
 *   scale_norm), bit 3 negate column flip_axis.  normal: rows with z < 0 are negated after the
 *   rotation and after the flip.  Steps run in bit order; the fused call is bit-identical to the
 *   same steps in separate calls (fixed fma order: csrc/augment.hip).
 * spt_augment_color_range_f32: range6 <- {min of columns 0..2, max of columns 0..2} of the
 *   (jittered, when jitter != 0) colours [n, 3]; integer atomics, bitwise reproducible; a NaN
 *   in a column makes its two records NaN.
 * spt_augment_color_f32: flags bit 0 jitter, bit 1 auto-contrast
 *   one_minus_blend * c + blend * ((c - lo) / (hi - lo)) with lo / hi from range6 (computed
 *   with the same seed), IEEE division, bit 2 c * 0.
 * ---------------------------------------------------------------------- */
int spt_augment_features_f32(const float* x, float* out, int64_t n, int n_cols, int64_t ld_x,
                             int64_t ld_out, int flags, uint64_t seed_jitter, double sigma,
                             double trunc, double lo, double hi, uint64_t col_mask,
                             uint64_t seed_rows, float p_rows, spt_stream_t stream);
int spt_augment_geometry_f32(const float* x, float* out, int64_t n, int64_t ld_x, int64_t ld_out,
                             int mode, int flags, uint64_t seed_jitter, double sigma, double trunc,
                             double lo, double hi, const float* rotation, const float* scale,
                             float scale_norm, int flip_axis, spt_stream_t stream);
int spt_augment_color_range_f32(const float* color, int64_t n, int64_t ld, int jitter,
                                uint64_t seed, double sigma, double trunc, double lo, double hi,
                                float* range6, spt_stream_t stream);
int spt_augment_color_f32(const float* color, float* out, int64_t n, int64_t ld_color,
                          int64_t ld_out, int flags, uint64_t seed, double sigma, double trunc,
                          double lo, double hi, const float* range6, float blend,
                          float one_minus_blend, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * GridSampling3D: voxel keys, one sort, one-pass groups        (csrc/voxel.hip)
 * GridSampling3D._process / _group_data (src/transforms/sampling.py:86-468).
 *
 * pos: f32, coordinate a of point i at pos[i * ld + a] (a block of a wider table works);
 * batch: int64 [n] or NULL; 1 <= n < 2^31.  The integer coordinate of a point is
 * rintf(pos / size): a correctly rounded IEEE f32 division, then round half to even - bit for
 * bit torch.round(pos / size).  Voxels are numbered in lexicographic order of
 * (batch, z, y, x), which is the order consecutive_cluster leaves of grid_cluster / voxel_grid.
 *
 * spt_voxel_bounds_f32: record = 10 device int32: min and max of x, y, z, min and max of
 *   batch (0, 0 without one), the number of points with a non-finite coordinate, the number of
 *   points with a coordinate or a batch index outside [-(2^31 - 1), 2^31 - 1].  Neither kind takes
 *   part in the bounds.  One set of integer atomics per workgroup; bitwise reproducible.
 * spt_voxel_groups_f32: the HOST hands back the minima (origin: x, y, z, batch) and the field
 *   widths (bits: x, y, z, batch; their sum in [1, 63]) it derived from the record.  Packs
 *   (batch, z, y, x) - origin into a u64 key, sorts (key, point) by a stable LSD radix sort over
 *   the significant bits only (low word, then high word when the key is wider than 32 bits),
 *   marks run heads, scans them and writes
 *     pointers [V + 1] int64 (capacity n + 1), cluster [n] int64 (voxel of every point),
 *     order [n] int64 (points sorted by voxel, ascending inside a voxel), last [V] int64
 *     (capacity n: highest point index of the voxel), coords [V, 3] int32 (capacity n; x, y, z,
 *     NOT shifted), *count = V (device int64).
 *   No kernel uses a key as an address.  ws: spt_voxel_groups_workspace_bytes(n, total bits).
 * spt_voxel_mean_f32: out[v * ld_out + c] = (sum of x[p * ld_x + c] over the voxel's points in
 *   ascending point order, from 0.0f) / (float)count - torch's CPU index_add arithmetic.  Runs
 *   longer than 512 points are summed by a whole wave: lane l adds elements l, l + 64, ... in
 *   order, then a fixed butterfly; no float atomics, bitwise reproducible either way.
 *   normalize != 0 (cols == 3): the row is then divided by sqrtf(x^2 + y^2 + z^2); a zero mean
 *   gives NaN, as the reference does.
 * spt_voxel_hist_i64: labels int64 [n], 1 <= n_bins <= 256.  hist (nullable) [V, n_bins] int64
 *   label counts; vote (nullable) [V] int64 = argmax of the counts, ties to the lowest label,
 *   without writing them.  A label outside [0, n_bins) sets *status (device int32) to 1 and is
 *   not counted.  Each row is owned by one lane or one wave: no global atomics.
 * spt_voxel_last: out [V] int64 = the point of the voxel with the greatest
 *   (rand32(seed, point), point); use_seed == 0: the highest point index.
 * ---------------------------------------------------------------------- */
int spt_voxel_bounds_f32(const float* pos, int64_t n, int64_t ld, float size,
                         const int64_t* batch, int32_t* record, spt_stream_t stream);
size_t spt_voxel_groups_workspace_bytes(int64_t n, int key_bits);
int spt_voxel_groups_f32(const float* pos, int64_t n, int64_t ld, float size,
                         const int64_t* batch, const int64_t* origin, const int* bits,
                         int64_t* pointers, int64_t* cluster, int64_t* order, int64_t* last,
                         int32_t* coords, int64_t* count, void* ws, size_t ws_bytes,
                         spt_stream_t stream);
int spt_voxel_mean_f32(const float* x, int64_t n, int cols, int64_t ld_x,
                       const int64_t* pointers, const int64_t* order, int64_t num_voxels,
                       int normalize, float* out, int64_t ld_out, spt_stream_t stream);
int spt_voxel_hist_i64(const int64_t* labels, int64_t n, const int64_t* pointers,
                       const int64_t* order, int64_t num_voxels, int n_bins, int64_t* hist,
                       int64_t* vote, int32_t* status, spt_stream_t stream);
int spt_voxel_last(const int64_t* pointers, const int64_t* order, int64_t n, int64_t num_voxels,
                   uint64_t seed, int use_seed, int64_t* out, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Predictions back to the cloud                                (csrc/predict.hip)
 * SemanticSegmentationOutput (src/utils/output_semantic.py) and the multi-run inference of
 * src/models/semantic.py:485-616.
 *
 * Every index and position is 64-bit; a size of 0 returns 0 without a launch; no entry reads
 * device memory from the host or resets a status record: status words are ADDED to, the caller
 * zeroes the record and reads it when it wants to know.  Nothing read from device memory is used
 * as an address before it is compared with its bound.
 *
 * spt_row_argmax_f32: logits f32 [rows, C], C >= 1.  pred (nullable) int64 [rows] =
 *   torch.argmax(logits, dim=1) bit for bit: the first maximum, a NaN above every number, the
 *   first NaN.  hist (nullable, with is_void) int64 [rows, ncols], void counts in the last
 *   column: is_void[r] (one byte, 0 / 1) = (float)hist[r, ncols - 1] / (float)sum(hist[r, :])
 *   > 0.5f, a correctly rounded f32 division of the two converted integers (0 / 0 = NaN: 0) -
 *   SemanticSegmentationOutput.void_mask.
 * spt_rows_accumulate_f32: acc f32 [N, C], src f32 [n, C], node_id int64 [n]:
 *   acc[node_id[i], :] = acc[node_id[i], :] + src[i, :], one f32 add per element (a[idx] += b
 *   for unique ids).  stamp int32 [N] (0 before the first run) takes run >= 1 by one atomic
 *   exchange per row; stamp != 0 is the reference's `seen`.  An id met twice in one run (the
 *   exchange returns run) is added once, by whichever occurrence came first, and counted in
 *   status[0]; an id outside [0, N) writes nothing and is counted in status[1].
 *   status: int32 [2].
 * spt_labels_by_index_i64: label int64 [num_label], idx_a int64 [n_a], idx_b (nullable) int64
 *   [n_b].  out_a (nullable) [n_a]: out_a[i] = label[idx_a[i]]; out_b (nullable) [n_b]:
 *   out_b[p] = label[idx_a[idx_b[p]]], in the same launch.  target (nullable, with confmat)
 *   int64 labels of the finest level present ([n_b] with idx_b, else [n_a]); confmat int64
 *   [C, C], 1 <= C <= 32: confmat[target, label] += 1 for both in [0, C) (anything else is
 *   void), ADDED to what the buffer holds by 64-bit integer atomics from a per-workgroup LDS
 *   table, non-zero cells only.  With confmat and both outputs NULL nothing of size n_b is
 *   written.  An index out of range gives -1, stays out of confmat and is counted:
 *   status[0] entries of idx_a outside [0, num_label), status[1] entries of idx_b outside
 *   [0, n_a).  status: int32 [4] (as below).
 * spt_labels_by_cluster_i64: the same from a Cluster (pointers int64 [num_clusters + 1], points
 *   int64 [num_points]) without its super_index: every position j in
 *   [pointers[v], pointers[v + 1]) gets out[points[j]] = label[idx_a ? idx_a[v] : v]; target /
 *   confmat as above with target indexed by points[j]; out (nullable) [num_points].  The work
 *   is cut by positions, 1 024 per workgroup pass, each pass finding its clusters by two
 *   searches of pointers: a cluster of thousands of points costs what thousands of singletons
 *   cost.  Empty clusters are legal.  status[0] entries of idx_a (or cluster numbers, without
 *   it) outside [0, num_label): -1 is written; status[1] entries of points outside
 *   [0, num_points): never written through; status[2] faults of pointers (a decreasing pair,
 *   pointers[0] != 0, pointers[num_clusters] != num_points): a position that no cluster
 *   claims is not written.  pointers are only compared, never used as an address.
 * ---------------------------------------------------------------------- */
int spt_row_argmax_f32(const float* logits, int64_t rows, int C, const int64_t* hist, int ncols,
                       int64_t* pred, uint8_t* is_void, spt_stream_t stream);
int spt_rows_accumulate_f32(float* acc, int64_t N, const float* src, const int64_t* node_id,
                            int64_t n, int C, int32_t* stamp, int run, int32_t* status,
                            spt_stream_t stream);
int spt_labels_by_index_i64(const int64_t* label, int64_t num_label, const int64_t* idx_a,
                            int64_t n_a, const int64_t* idx_b, int64_t n_b, int64_t* out_a,
                            int64_t* out_b, const int64_t* target, int C, int64_t* confmat,
                            int32_t* status, spt_stream_t stream);
int spt_labels_by_cluster_i64(const int64_t* label, int64_t num_label, const int64_t* idx_a,
                              const int64_t* pointers, const int64_t* points,
                              int64_t num_clusters, int64_t num_points, int64_t* out,
                              const int64_t* target, int C, int64_t* confmat, int32_t* status,
                              spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Panoptic evaluation                                          (csrc/panoptic.hip)
 * InstanceData.merge / iou_and_size / search_void / remove_void (src/data/instance.py), the
 * counters of PanopticQuality3D.compute (src/metrics/panoptic.py:225-323) and
 * scatter_mean_weighted (src/utils/scatter.py:17-38).
 *
 * An InstanceData is pointers int64 [G + 1] over P pairs (obj, count, y: int64 [P]).  P, G and
 * n are in 1 .. 2^31 - 2.  Grouping is one stable radix sort of a key as wide as its extents
 * need, run heads through the device scan and integer run sums: integer results are exact, no
 * float and no atomic whose order matters takes part.  No entry reads device memory from the
 * host; record / status words are ADDED to: the caller zeroes them and reads them when it wants
 * to know.  Nothing read from device memory is used as an address before it is compared with
 * its bound; pointers are searched and compared, or range-checked before a loop runs over them.
 * Runs (clusters, objects, groups) of more than 512 entries are reduced by a whole wave.
 *
 * spt_instance_extents_i64: record int64 [4] = min(obj), max(obj), min(idx), max(idx) (idx
 *   nullable; INT64_MAX / INT64_MIN where nothing was seen).  The record is initialised here.
 * spt_merge_instances_i64: pairs re-keyed by (idx[cluster], obj - obj_lo), obj_bits bits for
 *   the object (1 .. 62; obj_bits + bits(num_parents) <= 63), duplicates of a key become one
 *   pair with their counts summed, out CSR sorted by (parent, obj): out_pointers int64
 *   [num_parents + 1], out_obj / out_count / out_y int64 [P] of which the first record[0] are
 *   written; out_y is that of the LAST pair holding the key.  A parent without a pair gets an
 *   empty row.  record int64 [4]: [0] merged pairs, [1] parents with at least one pair, [2]
 *   pairs whose idx lies outside [0, num_parents) (merged into parent 0), [3] pairs that no
 *   cluster claims or whose obj lies outside [obj_lo, obj_lo + 2^obj_bits) (masked).
 * spt_pair_stats_i64: per pair a_size (points of its cluster), b_size (points of its object,
 *   plus cropped_in[pair] when given), iou f32 = (float)count / (float)(a_size + b_size - count),
 *   one correctly rounded division of the two converted integers; cluster_void [G] (bytes 0 / 1)
 *   = (float)void points / (float)points > 0.5f with void y < 0 or y >= C; pair_void = void
 *   object or void cluster; pair_cropped = points of the pair's object lying in void clusters
 *   (search_void).  kept_iou f32: the IoU of the pair AFTER remove_void(C) - the cluster without
 *   its void pairs, the object whole - and 0 for a void pair; gt_head: 1 on the last non-void
 *   pair of each object.  Objects are grouped by one sort of (obj - obj_lo, pair), obj_bits
 *   1 .. 63 (obj_lo = 0, obj_bits = 63 needs no knowledge of the extents).  Nothing is
 *   compacted.  status int32 [4]: [0] faults of pointers, [1] obj outside the key range.
 * spt_panoptic_counts_i64: state [5, C] 8-byte words, 1 <= C <= 32: rows tp, gt_count,
 *   pred_count int64, rows iou_sum, iou_mod_sum f64.  One pass over the pairs, one over the
 *   clusters, per-workgroup LDS tables flushed by 64-bit integer atomics.  A pair counts when
 *   pair_void is 0; gt_count[y] += gt_head; with pred_semantic[cluster] == y: iou > 0.5f
 *   (strictly) adds to tp and iou_sum, that or stuff_mask[y] to iou_mod_sum; pred_count
 *   [pred_semantic] += 1 per cluster with cluster_void 0.  The f64 sums are DETERMINISTIC by
 *   fixed point: each IoU is added as hi * 2^-32 + lo * 2^-64 into two 64-bit integers per sum
 *   (exact for every f32 in [2^-40, 1], enough for 2^31 pairs), and one f64 add per class and
 *   call brings them into the state.  status int32 [4]: [0] faults of pointers, [2]
 *   pred_semantic of a non-void cluster outside [0, C) (not counted), [3] IoUs outside [0, 1]
 *   (NaN of an empty union; not summed).
 * spt_weighted_group_mean_f32: out f32 [num_groups, cols] = sum(x[i] * w[i]) / sum(w[i]) over
 *   the rows with idx[i] == g: products rounded before they are added (no fma), both sums from
 *   0 in ascending row order, a zero weight sum replaced by 1, one division - the CPU result of
 *   scatter_mean_weighted bit for bit for groups of up to 512 rows; longer groups: exact f64
 *   products, 64 strided f64 partial sums, a fixed butterfly, one division and one rounding to
 *   f32.  status int32 [2]: [0] idx outside [0, num_groups).
 * ---------------------------------------------------------------------- */
int spt_instance_extents_i64(const int64_t* obj, int64_t P, const int64_t* idx, int64_t G,
                             int64_t* record, spt_stream_t stream);
size_t spt_merge_instances_workspace_bytes(int64_t P, int key_bits);
int spt_merge_instances_i64(const int64_t* pointers, const int64_t* obj, const int64_t* count,
                            const int64_t* y, const int64_t* idx, int64_t G, int64_t P,
                            int64_t num_parents, int64_t obj_lo, int obj_bits,
                            int64_t* out_pointers, int64_t* out_obj, int64_t* out_count,
                            int64_t* out_y, int64_t* record, void* ws, size_t ws_bytes,
                            spt_stream_t stream);
size_t spt_pair_stats_workspace_bytes(int64_t P, int64_t G, int key_bits);
int spt_pair_stats_i64(const int64_t* pointers, const int64_t* obj, const int64_t* count,
                       const int64_t* y, const int64_t* cropped_in, int64_t G, int64_t P, int C,
                       int64_t obj_lo, int obj_bits, int64_t* a_size, int64_t* b_size, float* iou,
                       uint8_t* cluster_void, uint8_t* pair_void, int64_t* pair_cropped,
                       float* kept_iou, uint8_t* gt_head, int32_t* status, void* ws,
                       size_t ws_bytes, spt_stream_t stream);
size_t spt_panoptic_counts_workspace_bytes(int C);
int spt_panoptic_counts_i64(int64_t* state, const int64_t* pred_semantic, const int64_t* pointers,
                            const int64_t* y, const uint8_t* pair_void, const float* kept_iou,
                            const uint8_t* gt_head, const uint8_t* cluster_void, int64_t G,
                            int64_t P, int C, const uint8_t* stuff_mask, int32_t* status, void* ws,
                            size_t ws_bytes, spt_stream_t stream);
size_t spt_weighted_group_mean_workspace_bytes(int64_t n, int64_t num_groups);
int spt_weighted_group_mean_f32(const float* x, int64_t n, int cols, const int64_t* idx,
                                const float* w, int64_t num_groups, float* out, int32_t* status,
                                void* ws, size_t ws_bytes, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Panoptic criterion: major objects                            (csrc/panoptic.hip)
 * InstanceData.major(num_classes) (src/data/instance.py:162-225) without a host read.
 *
 * spt_instance_major_i64: out_obj / out_count / out_y int64 [G], per cluster the pair of the
 *   largest count - ties to the lowest pair index.  A pair is void with y < 0 or y >= C.  If ANY
 *   cluster whose largest pair is void holds it with (float)count / (float)total <= 0.5f (one f32
 *   division of the converted integers; NaN counts as "not above"), EVERY cluster whose largest
 *   pair is void takes the pair of the largest count * ~void instead (ties to the lowest index; an
 *   all-void cluster takes its first pair with count 0) - as the reference's masked assignment
 *   behaves.  The decision stays a device flag: kernel 1 writes both candidates and ORs the flag,
 *   kernel 2 selects.  One lane per cluster, a whole wave for clusters of more than 64 pairs.
 *   status int32 [2], ADDED to: [0] clusters without a pair (the reference indexes out of range;
 *   here obj = -1, count = 0, y = -1), [1] faults of pointers (such a cluster is treated as
 *   empty).  Every access stays in bounds whatever the data.  G and P in 1 .. 2^31 - 2.
 * ---------------------------------------------------------------------- */
size_t spt_instance_major_workspace_bytes(int64_t G);
int spt_instance_major_i64(const int64_t* pointers, const int64_t* obj, const int64_t* count,
                           const int64_t* y, int64_t G, int64_t P, int C, int64_t* out_obj,
                           int64_t* out_count, int64_t* out_y, int32_t* status, void* ws,
                           size_t ws_bytes, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Superedges: subedges and the 7 stored edge features           (csrc/superedge.hip)
 * subedges (src/utils/graph.py:99-463) + _minimalistic_horizontal_edge_features
 * (src/transforms/graph.py:950-1060), one workgroup per edge, nothing expanded in memory.
 *
 * pos f32 [num_points, 3]; (perm, rowptr) the int32 CSR view of the point -> segment index;
 * edges int64, trimmed, row 0 at edges[0 .. E), row 1 at edges[edge_stride ..]; anchors int64
 * [2, E] dense (spt_cluster_pair_anchors_f32).  num_points <= 2^31 - 1, E and num_segments
 * below 2^31 - 1: refused otherwise.  Everything read from device memory (segment ids, row
 * pointers, anchors, point ids, offsets) is compared with its bound before it addresses
 * anything; an edge that fails a check gets count 0 and a zero row.
 *
 * spt_superedge_capacity: C, the most points a side of an edge may have in the workgroup
 *   kernel.  Classes: 0 = both sides 1 .. 64 points (a wave per edge), 1 = both sides 1 .. C
 *   (256 threads per edge, both sides in 32 KiB of LDS), 2 = everything else (the caller's
 *   composition).
 * spt_superedge_classify: order int32 [E] = the edge ids of class 0, then 1, then 2, each
 *   ascending; counts int64 [3].  Three flag arrays through the device scan.
 * spt_superedge_f32: the first num_small + num_medium entries of `order`.  switches: bit 0
 *   halfspace_filter, 1 bbox_filter, 2 target_pc_flip, 3 source_pc_sort.  count int32 [E] =
 *   st_k per edge.  count_only != 0 stops there (edge_attr, pairs, uid untouched).  Otherwise
 *   edge_attr f32 [E, 7] = mean_off, std_off (clipped to [-2, 2]), mean_dist; with pair_offset
 *   (uint32 [E + 1], spt_superedge_pair_offsets) the pairs of edge e go to pairs[0 / num_pairs +
 *   pair_offset[e] + rank] and uid likewise; without it no pair is written anywhere.  f32
 *   arithmetic in the order of graph.subedges, covariance and eigen-solve in f64; equal sort
 *   keys keep CSR order; sums are fixed trees of f64 partials, so runs are bit-equal.
 * spt_superedge_pair_offsets: offsets uint32 [E + 1] = exclusive scan of max(count, 0), total
 *   in the last slot (the caller guarantees it is below 2^32).  ws: at least
 *   spt_superedge_workspace_bytes(E), which covers classify too.
 * ---------------------------------------------------------------------- */
int spt_superedge_capacity(void);
size_t spt_superedge_workspace_bytes(int64_t num_edges);
int spt_superedge_classify(const int32_t* rowptr, int64_t num_segments, const int64_t* edges,
                           int64_t num_edges, int64_t edge_stride, int32_t* order,
                           int64_t* counts, void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_superedge_pair_offsets(const int32_t* count, int64_t num_edges, uint32_t* offsets,
                               void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_superedge_f32(const float* pos, int64_t num_points, const int32_t* perm,
                      const int32_t* rowptr, int64_t num_segments, const int64_t* edges,
                      int64_t num_edges, int64_t edge_stride, const int64_t* anchors,
                      const int32_t* order, int64_t num_small, int64_t num_medium, float ratio,
                      int k_min, float margin, int switches, int count_only, float* edge_attr,
                      int32_t* count, const uint32_t* pair_offset, int64_t* pairs, int64_t* uid,
                      int64_t num_pairs, spt_stream_t stream);

/* ------------------------------------------------------------------------
 * Greedy contour-prior partition                                  (merge.hip)
 * The merge rounds of GreedyContourPriorPartition (src/transforms/partition.py:383-653,
 * src/utils/components.py:11-130; the reference's loop lives in torch_graph_components, so the
 * rounds are this project's own: DESIGN 7.22).  Component state: size int64 [C], feat f64
 * [C, d] = sum of s_i x_i, pos f64 [C, 3] = sum of s_i pos_i.  No float atomics anywhere:
 * every output is bitwise reproducible.  Sums over more than 512 members are 64 strided partial
 * sums combined by the xor tree 32, 16, .., 1; shorter ones run serially from the first member.
 *
 * spt_component_graph_f32: quotient of an edge list (rows at [0..E) and [edge_stride..), any
 *   order, both directions, duplicates, self loops) under index [num_nodes] (nullable =
 *   identity, then num_components == num_nodes): ends relabelled, ordered lo < hi, lo == hi
 *   dropped, sorted by (lo, hi) with a stable radix sort, equal pairs merged with reduce
 *   (0 add, 1 mean, 2 max, 3 min, 4 mul) in f32 in input order.  edge_attr nullable = ones.
 *   out_edges rows at [0..) and [out_stride..), out_attr: room for E entries, the first
 *   counts[0] are written.  counts int64 [2]: edges out, edges with an end out of range
 *   (dropped).
 * spt_merge_means_f64: mean [C, d] = feat / size.
 * spt_merge_choose_f64: per edge (a, b, w) of a component graph, g = f32(s_a s_b / (s_a + s_b)
 *   * |m_a - m_b|^2 - reg * w) in f64 (the squares summed from column 0), and best [C] uint64 =
 *   min over the edges at the component of (orderable bits of g) << 32 | other end; all ones
 *   where the component has no edge.  gain f32 [E] nullable.
 * spt_merge_resolve: a is active iff it has an edge and (size < min_size, or not
 *   merge_only_small and g < 0).  parent [C] = the choice of an active a, else a; of two active
 *   components that chose each other the smaller is its own parent.  active: device int64 count.
 * spt_merge_jump: out [C] = parent[parent[.]] (out != parent); changed (nullable) device int64,
 *   set to 1 when an entry moved, else 0.
 * spt_merge_accumulate_f64: label [num_old] in [0, num_new), every new id used.  Sizes, feature
 *   rows and (pos nullable, with pos_out) position rows summed per new id over its members in
 *   ascending old id.
 * spt_edge_weights_f32: dist [E] = f32(sqrt(sum_c (rows[a, c] - rows[b, c])^2)) in f64 from
 *   column 0, rows f32 [num_nodes, cols] with leading dimension ld; sum: device f64 sum of dist
 *   in a fixed order; bad: device int64 count of edges with an end out of range (dist 0).
 * ---------------------------------------------------------------------- */
size_t spt_component_graph_workspace_bytes(int64_t num_edges);
int spt_component_graph_f32(const int64_t* edge_index, int64_t num_edges, int64_t edge_stride,
                            const float* edge_attr, const int64_t* index, int64_t num_nodes,
                            int64_t num_components, int reduce, int64_t* out_edges,
                            int64_t out_stride, float* out_attr, int64_t* counts, void* ws,
                            size_t ws_bytes, spt_stream_t stream);
int spt_merge_means_f64(const double* feat, const int64_t* size, int64_t num_components, int d,
                        double* mean, spt_stream_t stream);
int spt_merge_choose_f64(const double* mean, const int64_t* size, int64_t num_components, int d,
                         const int64_t* edges, int64_t num_edges, int64_t edge_stride,
                         const float* weights, double reg, uint64_t* best, float* gain,
                         spt_stream_t stream);
int spt_merge_resolve(const uint64_t* best, const int64_t* size, int64_t num_components,
                      int64_t min_size, int merge_only_small, int64_t* parent, int64_t* active,
                      spt_stream_t stream);
int spt_merge_jump(const int64_t* parent, int64_t num_components, int64_t* out, int64_t* changed,
                   spt_stream_t stream);
size_t spt_merge_accumulate_workspace_bytes(int64_t num_old, int64_t num_new);
int spt_merge_accumulate_f64(const int64_t* label, int64_t num_old, int64_t num_new,
                             const int64_t* size, const double* feat, int d, const double* pos,
                             int64_t* size_out, double* feat_out, double* pos_out, void* ws,
                             size_t ws_bytes, spt_stream_t stream);
size_t spt_edge_weights_workspace_bytes(int64_t num_edges);
int spt_edge_weights_f32(const float* rows, int64_t num_nodes, int cols, int64_t ld,
                         const int64_t* edge_index, int64_t num_edges, int64_t edge_stride,
                         float* dist, double* sum, int64_t* bad, void* ws, size_t ws_bytes,
                         spt_stream_t stream);

/* ----------------------------------------------------------------------
 * Stride-1 sparse 3D convolution (csrc/sparse_conv.hip).
 *   out[i] = bias + sum over o ascending of x[j(i, o)] W[o],  W [K^3, c_in, c_out] row-major,
 *   o = ((dz + r) K + (dy + r)) K + (dx + r), j(i, o) the voxel of i's batch item at
 *   coords[i] + d (dx, dy, dz).  coords int32 [n, 3] (x, y, z), batch int64 [n] nullable.
 *
 * spt_sparse_bounds_i32: record int64 [8] = min, max of x, y, z, batch (0, 0 without a batch).
 * Key layout (host arrays): origin[4] = the minimum of x, y, z MINUS r d, and of batch; bits[4]
 *   = the width of (max - min + 2 r d) for x, y, z and of (max - min) for batch; 1 .. 63 bits in
 *   all.  The padding is what keeps a neighbour position outside the bounds from meeting another
 *   voxel's key; a layout that does not cover the data gives a wrong map, never a stray access.
 * spt_sparse_map_count: sorts the keys, leaves skeys [n] / sorder [n] (sorted keys and the voxel
 *   of each), rowptr [n + 1] (exclusive scan of the pairs per voxel), record int64 [2] = number
 *   of pairs (64-bit: check it before rowptr is trusted), number of duplicate (batch, coords).
 * spt_sparse_map_fill: the pairs of voxel i at [rowptr[i], rowptr[i + 1]), offsets ascending:
 *   nbr (the neighbour j), off (the offset index o), row (i); num_pairs = rowptr[n].
 * spt_sparse_map_by_offset: perm [P] = the pairs stably sorted by offset, optr [k3 + 1] the run
 *   of each offset (for dW).
 * spt_sparse_conv_fwd_f32: c_in, c_out 1 .. 64 (the Python route hands it c_out % 16 == 0, which
 *   spt_sparse_conv_supported answers; the dX call hands it the transposed shape).  flip != 0
 *   reads W[k3 - 1 - o]: with w = W transposed per offset [k3, c_out, c_in] and x = gout it is
 *   dX, on the same map.  bias nullable.  f32 matrix pipe, no atomics, each row written once.
 * spt_sparse_conv_dw_f32: dw [k3, c_in, c_out], dw[o] = sum over the pairs of o in ascending
 *   pair order of x[nbr]^T gout[row]: 64 fixed chunks per offset, then added in order.
 * spt_sparse_conv_dbias_f32: dbias [c_out] = column sums of gout: 1024 fixed row ranges, then
 *   added in order.
 * Given a built map, fwd, dw and dbias read nothing back to the host.
 * ---------------------------------------------------------------------- */
int spt_sparse_bounds_i32(const int32_t* coords, const int64_t* batch, int64_t n, int64_t* record,
                          spt_stream_t stream);
size_t spt_sparse_map_count_workspace_bytes(int64_t n, int key_bits);
int spt_sparse_map_count(const int32_t* coords, const int64_t* batch, int64_t n,
                         const int64_t* origin, const int* bits, int kernel_size, int dilation,
                         uint64_t* skeys, int32_t* sorder, int32_t* rowptr, int64_t* record,
                         void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_sparse_map_fill(const int32_t* coords, const int64_t* batch, int64_t n,
                        const int64_t* origin, const int* bits, int kernel_size, int dilation,
                        const uint64_t* skeys, const int32_t* sorder, const int32_t* rowptr,
                        int64_t num_pairs, int32_t* nbr, int32_t* off, int32_t* row,
                        spt_stream_t stream);
size_t spt_sparse_map_by_offset_workspace_bytes(int64_t num_pairs);
int spt_sparse_map_by_offset(const int32_t* off, int64_t num_pairs, int k3, int32_t* perm,
                             int32_t* optr, void* ws, size_t ws_bytes, spt_stream_t stream);
int spt_sparse_conv_supported(int c_in, int c_out);
int spt_sparse_conv_fwd_f32(const float* x, int64_t n, int c_in, const float* w, int k3, int c_out,
                            const float* bias, const int32_t* rowptr, const int32_t* nbr,
                            const int32_t* off, int flip, float* out, spt_stream_t stream);
size_t spt_sparse_conv_dw_workspace_bytes(int k3, int c_in, int c_out);
int spt_sparse_conv_dw_f32(const float* x, const float* gout, int64_t n, int c_in, int c_out,
                           int k3, const int32_t* nbr, const int32_t* row, const int32_t* perm,
                           const int32_t* optr, int64_t num_pairs, float* dw, void* ws,
                           size_t ws_bytes, spt_stream_t stream);
size_t spt_sparse_conv_dbias_workspace_bytes(int c_out);
int spt_sparse_conv_dbias_f32(const float* gout, int64_t n, int c_out, float* dbias, void* ws,
                              size_t ws_bytes, spt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SPT_HIP_H */
