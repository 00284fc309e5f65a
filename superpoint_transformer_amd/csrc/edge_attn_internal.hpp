// What the four attention files (edge_attn.hip: C entry points, mode word, route; edge_attn_mfma.hip,
// edge_attn_el.hip, edge_attn_to.hip: the matrix-pipe kernels and their launchers) share.
#pragma once

#include <stdlib.h>

#include "common.hpp"

namespace spt {

// ---- fields of a RESOLVED mode word (spt_attn_resolve_mode, include/spt_hip.h) -------------------
static inline int attn_mode_precision(int word) { return word & 3; }
static inline int attn_mode_form(int word) { return word & (3 << 4); }     // SPT_ATTN_BWD_*
static inline bool attn_mode_target_order(int word) { return (word & (3 << 6)) == SPT_ATTN_BWD_TARGET_ORDER; }
// ABI precision (SPT_ATTN_F32 / _SPLIT_BF16 / _BF16) -> the matrix-pipe kernels' PREC parameter:
// 0 f32 pipe, 3 split-bf16 (three bf16 products per f32 product), 1 plain bf16 operands
static inline int attn_kernel_prec(int precision) { return precision == 2 ? 3 : (precision == 3 ? 1 : 0); }

// XCD bands of the attention kernels' work distribution (edge_attn_mfma.hip forward, edge_attn_to.hip
// backward): a SPEED choice between two walks of the same work - read once from the environment
// (SPT_ATTN_XCD_BANDS=0 restores the plain grid stride / contiguous tile ranges for A/B runs).
inline bool attn_xcd_bands() {
  static const bool on = [] { const char* e = getenv("SPT_ATTN_XCD_BANDS"); return e ? atoi(e) != 0 : true; }();
  return on;
}

// ---- edge_attn_mfma.hip: matrix-pipe formulation for the SPT-64 head layout ----------------------
// (the shape these kernels are built for; has_rpe = edge_attr and all three encoders)
bool attn_mfma_shape_ok(int H, int D, int Dv, int F, bool has_rpe);
void attn_fwd_mfma_launch(const float* qkv, int64_t n, const int32_t* erowptr,
                          const int32_t* eperm, const int32_t* tgt, const float* ea,
                          const float* Wk, const float* bk, const float* Wq, const float* bq,
                          const float* Wv, const float* bv, int scale_mode, float scale_a,
                          float* out, float* m, float* z, int split_bf16, hipStream_t stream);
// (the backward launchers return the number of partial weight-gradient tables they wrote)
int attn_bwd_mfma_launch(const float* qkv, int64_t n, const int32_t* erowptr,
                         const int32_t* eperm, const int32_t* tgt, const float* ea,
                         const float* Wk, const float* bk, const float* Wq, const float* bq,
                         const float* Wv, const float* bv, int scale_mode, float scale_a,
                         const float* out, const float* m, const float* z, const float* gout,
                         float* gqkv, float* gea, int gea_acc, float* partial, int split_bf16,
                         int64_t e, int packed, hipStream_t stream);

// ---- edge_attn_el.hip: edge-lane backward over the edge stream in SOURCE order -------------------
size_t attn_bwd_el_workspace_bytes(int64_t n, int64_t e);
void attn_pack_tile_ids_launch(const int32_t* eperm, const int32_t* tgt, const int32_t* src,
                               int64_t e, int32_t* ids3, hipStream_t stream);
int attn_bwd_el_launch(const float* qkv, int64_t n, const int32_t* erowptr, const int32_t* eperm,
                       const int32_t* tgt, const int32_t* src, const int32_t* tile_ids,
                       const int32_t* tperm, const int32_t* trowptr, int64_t e, const float* ea,
                       const float* Wk, const float* bk, const float* Wq, const float* bq,
                       const float* Wv, const float* bv, int scale_mode, float scale_a,
                       const float* out, const float* m, const float* z, const float* gout,
                       float* gqkv, float* gea, int gea_acc, float* partial, void* ws, int prec,
                       hipStream_t stream);

// ---- edge_attn_to.hip: the same backward over the edge stream in TARGET order --------------------
size_t attn_bwd_to_workspace_bytes(int64_t n, int64_t e);
void attn_pack_tile_ids_to_launch(const int32_t* eperm, const int32_t* tgt, const int32_t* src,
                                  const int32_t* tperm, int64_t e, int32_t* ids4, hipStream_t stream);
int attn_mirror_prepare_launch(const int64_t* ei, const int32_t* eperm, int64_t e, int64_t pairs,
                               int32_t* inv, int32_t* flag, hipStream_t stream);
void attn_pack_tile_ids_mirror_launch(const int32_t* eperm, const int32_t* tgt, const int32_t* src,
                                      const int32_t* inv, int64_t e, int64_t pairs, int32_t* ids4,
                                      hipStream_t stream);
int attn_bwd_to_launch(const float* qkv, int64_t n, const int32_t* erowptr, const int32_t* eperm,
                       const int32_t* tgt, const int32_t* src, const int32_t* tile_ids,
                       const int32_t* tperm, int64_t e, const float* ea, const float* Wk,
                       const float* bk, const float* Wq, const float* bq, const float* Wv,
                       const float* bv, int scale_mode, float scale_a, const float* out,
                       const float* m, const float* z, const float* gout, float* gqkv, float* gea,
                       int gea_acc, float* partial, void* ws, int prec, hipStream_t stream);

}  // namespace spt
