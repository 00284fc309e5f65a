"""ctypes binding of libspt_hip.so (C ABI declared in include/spt_hip.h).

The library is the product: there is NO CPU or PyTorch fallback.  Importing
this module without the built shared object raises, and every wrapper raises
``RuntimeError`` with ``spt_last_error()`` on a non-zero status.
"""
import ctypes
import os

import torch  # noqa: F401  (loads torch's libamdhip64.so.7 first so ours binds to it)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libspt_hip.so")

_c = ctypes
_i64 = _c.c_int64
_int = _c.c_int
_p = _c.c_void_p
_sz = _c.c_size_t
_f32 = _c.c_float
_f64 = _c.c_double

# name -> (restype, argtypes).  Must list EVERY symbol of include/spt_hip.h:
# tests/test_abi.py parses the header and checks both directions.
SIGNATURES = {
    "spt_version": (_int, []),
    "spt_last_error": (_c.c_char_p, []),
    "spt_csr_build_workspace_bytes": (_sz, [_i64, _i64]),
    "spt_csr_build": (_int, [_p, _i64, _i64, _p, _p, _p, _sz, _p]),
    "spt_csr_pos_seg": (_int, [_p, _i64, _i64, _p, _p]),
    "spt_csr_gather_i64_i32": (_int, [_p, _p, _i64, _p, _p]),
    "spt_edge_csr_build_workspace_bytes": (_sz, [_i64, _i64]),
    "spt_edge_csr_build": (_int, [_p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "spt_segcsr_reduce_f32": (_int, [_int, _p, _p, _p, _i64, _i64, _int, _p, _p, _p]),
    "spt_segcsr_max_affine_f32": (_int, [_p, _p, _p, _i64, _i64, _int, _p, _p, _p, _f32, _p, _p, _p, _p]),
    "spt_segcsr_max_affine_bf16_supported": (_int, [_int, _i64]),
    "spt_segcsr_max_affine_bf16": (_int, [_p, _p, _p, _i64, _i64, _int, _p, _p, _p, _f32, _p, _p, _p, _p]),
    "spt_segcsr_max_affine_raw_supported": (_int, [_int, _i64]),
    "spt_segcsr_max_affine_raw_f32": (_int, [_p, _int, _p, _p, _i64, _i64, _int, _p, _p, _p, _f32, _p, _p, _p,
                                             _p, _p]),
    "spt_graphnorm_bwd_stats_sparse_raw_f32": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _int, _int, _p, _p, _p,
                                                      _f32, _p, _p, _sz, _p]),
    "spt_fused_linear_storage_supported": (_int, [_int, _int]),
    "spt_graphnorm_bwd_stats_sparse_ex_f32": (_int, [_p, _int, _p, _p, _p, _p, _i64, _i64, _int, _int, _p, _p,
                                                     _p, _f32, _p, _p, _sz, _p]),
    "spt_segcsr_reduce_bwd_f32": (_int, [_int, _p, _p, _p, _p, _p, _i64, _i64, _int, _p, _p]),
    "spt_segcsr_sum_i64": (_int, [_p, _p, _p, _i64, _i64, _int, _p, _p]),
    "spt_gather_rows_f32": (_int, [_p, _p, _i64, _i64, _int, _p, _p]),
    "spt_graphnorm_workspace_bytes": (_sz, [_i64, _int, _int]),
    "spt_graphnorm_fwd_f32": (_int, [_p, _p, _i64, _int, _int, _p, _p, _p, _f32, _f32,
                                     _p, _p, _p, _p, _sz, _p]),
    "spt_graphnorm_bwd_f32": (_int, [_p, _p, _p, _i64, _int, _int, _p, _p, _p, _p, _p,
                                     _f32, _p, _p, _p, _p, _p, _sz, _p]),
    "spt_graphnorm_stats_f32": (_int, [_p, _p, _i64, _int, _int, _p, _p, _f32, _p, _p, _p, _p,
                                       _p, _sz, _p]),
    "spt_graphnorm_bwd_acc_f32": (_int, [_p, _p, _p, _i64, _int, _int, _p, _p, _p, _p, _p,
                                         _f32, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "spt_edge_attn_fwd_f32": (_int, [_p, _i64, _int, _int, _int, _p, _p, _p, _i64, _p, _int,
                                     _p, _p, _p, _p, _p, _p, _int, _f32, _p, _p, _p, _p]),
    "spt_edge_attn_bwd_workspace_bytes": (_sz, [_int, _int, _int, _int]),
    "spt_attn_use_mfma": (_int, [_int]),
    "spt_attn_bwd_packed": (_int, [_int]),
    "spt_attn_bwd_el_full_line": (_int, [_int]),
    "spt_attn_bwd_el_target_order": (_int, [_int]),
    "spt_attn_tile_record_ints": (_int, []),
    "spt_attn_pack_tile_ids_ex": (_int, [_p, _p, _p, _p, _i64, _p, _p]),
    "spt_attn_tile_record_ints_m": (_int, [_int]),
    "spt_attn_pack_tile_ids_m": (_int, [_p, _p, _p, _p, _i64, _int, _p, _p]),
    "spt_attn_mirror_prepare": (_int, [_p, _p, _i64, _i64, _p, _p, _p]),
    "spt_attn_pack_tile_ids_mirror": (_int, [_p, _p, _p, _p, _i64, _i64, _p, _p]),
    "spt_attn_split_pack_f32": (_int, [_p, _i64, _int, _int, _p, _p]),
    "spt_attn_split_grad_f32": (_int, [_p, _i64, _int, _int, _p, _p]),
    "spt_edge_attn_bwd_f32": (_int, [_p, _i64, _int, _int, _int, _p, _p, _p, _i64, _p, _int,
                                     _p, _p, _p, _p, _p, _p, _int, _f32, _p, _p, _p, _p,
                                     _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "spt_edge_attn_bwd_acc_f32": (_int, [_p, _i64, _int, _int, _int, _p, _p, _p, _i64, _p, _int,
                                         _p, _p, _p, _p, _p, _p, _int, _f32, _p, _p, _p, _p,
                                         _p, _p, _int, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "spt_edge_attn_fwd_ex_f32": (_int, [_p, _i64, _int, _int, _int, _p, _p, _p, _i64, _p, _int,
                                        _p, _p, _p, _p, _p, _p, _int, _f32, _p, _p, _p, _int, _p]),
    "spt_attn_resolve_mode": (_int, [_int]),
    "spt_edge_attn_bwd_route": (_int, [_i64, _i64, _int, _int, _int, _int, _int, _int, _sz]),
    "spt_edge_attn_bwd_ex_workspace_bytes": (_sz, [_i64, _i64, _int, _int, _int, _int]),
    "spt_edge_attn_bwd_el_supported": (_int, [_int, _int, _int, _int, _int]),
    "spt_attn_pack_tile_ids": (_int, [_p, _p, _p, _i64, _p, _p]),
    "spt_edge_attn_bwd_ex_f32": (_int, [_p, _i64, _int, _int, _int, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _int,
                                        _p, _p, _p, _p, _p, _p, _int, _f32, _p, _p, _p, _p,
                                        _p, _p, _int, _p, _p, _p, _p, _p, _p, _int, _p, _sz, _p]),
    "spt_grid_knn_workspace_bytes": (_sz, [_i64, _i64]),
    "spt_knn_use_cell_path": (_int, [_int]),
    "spt_segcsr_use_stream": (_int, [_int]),
    "spt_segcsr_reduce_ex_f32": (_int, [_int, _p, _p, _p, _i64, _i64, _int, _p, _p, _int, _p]),
    "spt_segcsr_max_affine_ex_f32": (_int, [_p, _p, _p, _i64, _i64, _int, _p, _p, _p, _f32, _p, _p, _p,
                                            _int, _p]),
    "spt_grid_knn_ex_f32": (_int, [_p, _i64, _p, _i64, _int, _f32, _f32, _p, _p, _int, _int, _int,
                                   _p, _p, _p, _int, _p, _sz, _p]),
    "spt_grid_knn_geof_f32": (_int, [_p, _i64, _int, _f32, _f32, _p, _p, _int, _int, _int, _int,
                                     _p, _p, _p, _p, _int, _p, _sz, _p]),
    "spt_grid_knn_after_f32": (_int, [_p, _i64, _p, _i64, _int, _f32, _f32, _p, _p, _int, _int, _p, _p,
                                      _p, _p, _p, _sz, _p]),
    "spt_grid_knn_f32": (_int, [_p, _i64, _p, _i64, _int, _f32, _f32, _p, _p, _int, _int, _int,
                                _p, _p, _p, _p, _sz, _p]),
    "spt_point_geof_dense_f32": (_int, [_p, _i64, _p, _int, _int, _int, _int, _p, _p, _p]),
    "spt_point_geof_dense_ld_f32": (_int, [_p, _i64, _p, _int, _i64, _int, _int, _int, _p, _p, _p]),
    "spt_bbox_f32": (_int, [_p, _i64, _p, _p]),
    "spt_knn_subsample_f32": (_int, [_p, _i64, _p, _f32, _int, _p, _p, _p]),
    "spt_grid_cell_ids_f32": (_int, [_p, _i64, _f32, _p, _p, _p, _p]),
    "spt_grid_count_cells_workspace_bytes": (_sz, [_i64]),
    "spt_grid_count_cells_f32": (_int, [_p, _i64, _f32, _p, _p, _p, _p, _sz, _p]),
    "spt_spatial_order_workspace_bytes": (_sz, [_i64, _i64]),
    "spt_spatial_order": (_int, [_p, _i64, _f32, _p, _p, _p, _p, _sz, _p]),
    "spt_point_geof_csr_f32": (_int, [_p, _i64, _p, _p, _int, _int, _int, _p, _p]),
    "spt_vertical_edge_features_f32": (_int, [_p, _i64] + [_p] * 13 + [_p]),
    "spt_edge_affinity_features_f32": (_int, [_p, _i64, _int, _p, _p, _i64, _p, _p]),
    "spt_edge_affinity_features_bwd_f32": (_int, [_p, _p, _i64, _int, _p, _p, _i64, _p, _p]),
    "spt_scatter_pca_f32": (_int, [_p, _p, _p, _i64, _p, _p, _p]),
    "spt_neighbors_dense_to_csr_workspace_bytes": (_sz, [_i64]),
    "spt_neighbors_dense_to_csr": (_int, [_p, _i64, _int, _p, _p, _p, _p, _sz, _p]),
    "spt_horizontal_edge_features_f32": (_int, [_p, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _int,
                                                _p, _p, _p]),
    "spt_graphnorm_tables_f32": (_int, [_p, _int, _int, _p, _p, _f32, _p, _p, _p, _p, _p]),
    "spt_graphnorm_apply_f32": (_int, [_p, _p, _i64, _int, _int, _p, _p, _p, _f32, _p, _p]),
    "spt_graphnorm_bwd_stats_f32": (_int, [_p, _p, _p, _i64, _int, _int, _p, _p, _p, _f32, _p,
                                           _p, _sz, _p]),
    "spt_graphnorm_bwd_stats_sparse_workspace_bytes": (_sz, [_i64, _int, _int]),
    "spt_graphnorm_bwd_stats_sparse_f32": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _int, _int, _p, _p,
                                                   _p, _f32, _p, _p, _sz, _p]),
    "spt_graphnorm_bwd_tables_f32": (_int, [_p, _int, _int, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                            _p, _p]),
    "spt_fused_linear_supported": (_int, [_int, _int]),
    "spt_fused_linear_use_split_bf16": (_int, [_int]),
    "spt_fused_linear_bwd_use_dma": (_int, [_int]),
    "spt_fused_linear_bwd_route": (_int, [_int, _int, _int, _int]),
    "spt_fused_linear_fwd_use_x3": (_int, [_int]),
    "spt_fused_linear_pooled_supported": (_int, [_int, _int]),
    "spt_fused_linear_bwd_pooled_f32": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _int, _p, _p, _p, _f32,
                                               _p, _p, _p, _p, _int, _p, _p, _p, _f32, _p, _p, _p,
                                               _int, _p, _p, _sz, _p]),
    "spt_fused_linear_pooled_supported_ex": (_int, [_int, _int, _int]),
    "spt_fused_linear_fwd_ex_f32": (_int, [_p, _i64, _i64, _int, _p, _int, _p, _p, _p, _f32, _p, _p,
                                           _int, _p, _sz, _p]),
    "spt_fused_linear_bwd_ex_f32": (_int, [_p, _p, _i64, _i64, _int, _p, _p, _p, _f32, _p, _p, _p,
                                           _p, _int, _p, _p, _p, _f32, _p, _p, _p, _int, _p, _int, _p,
                                           _sz, _p]),
    "spt_fused_linear_bwd_pooled_ex_f32": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _int, _p, _p, _p, _f32,
                                                  _p, _p, _p, _p, _int, _p, _p, _p, _f32, _p, _p, _p,
                                                  _int, _p, _int, _p, _sz, _p]),
    "spt_fused_linear_workspace_bytes": (_sz, [_int, _int]),
    "spt_fused_linear_fwd_runs_f32": (_int, [_p, _int, _p, _p, _p, _int, _int, _p, _int, _p, _p, _p,
                                             _f32, _p, _p, _int, _p, _sz, _p]),
    "spt_fused_linear_bwd_runs_f32": (_int, [_p, _p, _int, _p, _p, _p, _int, _int, _p, _p, _p, _f32,
                                             _p, _p, _p, _p, _int, _p, _p, _p, _f32, _p, _p, _p, _p,
                                             _int, _p, _sz, _p]),
    "spt_fused_linear_bwd_pooled_runs_f32": (_int, [_p, _p, _p, _p, _p, _int, _p, _p, _p, _int, _int,
                                                    _p, _p, _p, _f32, _p, _p, _p, _p, _int, _p, _p,
                                                    _p, _f32, _p, _p, _p, _p, _int, _p, _sz, _p]),
    "spt_fused_linear_fwd_runs_gn_f32": (_int, [_p, _int, _p, _p, _p, _int, _int, _p, _int, _p, _p, _p,
                                                _f32, _p, _p, _int, _p, _sz, _p, _p]),
    "spt_fused_linear_bwd_runs_gn_f32": (_int, [_p, _p, _int, _p, _p, _p, _int, _int, _p, _p, _p, _f32,
                                                _p, _p, _p, _p, _int, _p, _p, _p, _f32, _p, _p, _p, _p,
                                                _int, _p, _sz, _p, _p]),
    "spt_fused_linear_bwd_fold_supported": (_int, [_int, _int, _int, _int]),
    "spt_fused_linear_bwd_runs_gn_fold_f32": (_int, [_p, _p, _int, _p, _p, _p, _int, _int, _p, _p, _p, _f32,
                                                     _p, _p, _p, _p, _int, _p, _p, _p, _f32, _p, _p,
                                                     _int, _p, _sz, _p, _p, _int, _p, _p, _p]),
    "spt_fused_linear_bwd_pooled_runs_gn_f32": (_int, [_p, _p, _p, _p, _p, _int, _p, _p, _p, _int, _int,
                                                       _p, _p, _p, _f32, _p, _p, _p, _p, _int, _p, _p,
                                                       _p, _f32, _p, _p, _p, _p, _int, _p, _sz, _p, _p]),
    "spt_fused_linear_bwd_pool_runs_gn_f32": (_int, [_p, _p, _p, _p, _p, _p, _i64, _int, _p, _p, _p, _int,
                                                     _int, _p, _p, _p, _f32, _p, _p, _p, _p, _int, _p, _p,
                                                     _p, _f32, _p, _p, _p, _p, _p, _p, _int, _p, _sz, _p, _p]),
    "spt_csr_check_i64": (_int, [_p, _p, _p, _i64, _i64, _int, _p, _p]),
    "spt_csr_adopt_i64": (_int, [_p, _p, _p, _i64, _i64, _p, _p, _p, _p]),
    "spt_fused_linear_pool_supported": (_int, [_int, _int, _int]),
    "spt_fused_linear_pool_gram_len": (_sz, [_int]),
    "spt_fused_linear_pool_workspace_bytes": (_sz, [_int, _int]),
    "spt_fused_linear_fwd_pool_runs_f32": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _int, _p, _p, _p, _int,
                                                  _int, _p, _int, _p, _p, _p, _f32, _f32, _p, _p, _p,
                                                  _f32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _int, _p,
                                                  _sz, _p]),
    "spt_fused_linear_bwd_pool_runs_f32": (_int, [_p, _p, _p, _p, _p, _p, _i64, _int, _p, _p, _p, _int,
                                                  _int, _p, _p, _p, _f32, _p, _p, _p, _p, _int, _p, _p,
                                                  _p, _f32, _p, _p, _p, _p, _p, _p, _int, _p, _sz, _p]),
    "spt_fused_linear_fwd_f32": (_int, [_p, _i64, _i64, _int, _p, _int, _p, _p, _p, _f32, _p, _p,
                                        _p, _sz, _p]),
    "spt_fused_linear_bwd_f32": (_int, [_p, _p, _i64, _i64, _int, _p, _p, _p, _f32, _p, _p, _p,
                                        _p, _int, _p, _p, _p, _f32, _p, _p, _p, _int, _p, _p,
                                        _sz, _p]),
    "spt_unit_sphere_norm_f32": (_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _p]),
    "spt_unit_sphere_assemble_f32": (_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _p, _int, _p, _p, _p, _p]),
    "spt_unit_sphere_workspace_bytes": (_sz, [_i64, _i64]),
    "spt_unit_sphere_norm_ws_f32": (_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _p, _sz, _p]),
    "spt_unit_sphere_assemble_ws_f32": (_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _p, _int, _p, _p, _p,
                                               _p, _sz, _p]),
    "spt_sparse_sample_workspace_bytes": (_sz, [_i64, _i64]),
    "spt_sparse_sample": (_int, [_p, _i64, _i64, _p, _int, _int, _c.c_uint64, _p, _p, _p, _sz, _p]),
    "spt_segment_std_f32": (_int, [_p, _p, _p, _i64, _int, _p, _p]),
    "spt_segment_mean_orientation_f32": (_int, [_p, _p, _p, _i64, _p, _p]),
    "spt_cluster_graph_edges_workspace_bytes": (_sz, [_i64, _int]),
    "spt_cluster_graph_edges": (_int, [_p, _p, _p, _i64, _int, _f32, _int, _p, _p, _p, _p, _sz, _p]),
    "spt_skinny_linear_supported": (_int, [_int, _int]),
    "spt_narrow_linear_bwd_supported": (_int, [_int, _int]),
    "spt_narrow_linear_bwd_workspace_bytes": (_sz, [_int, _int]),
    "spt_narrow_linear_bwd_f32": (_int, [_p, _p, _p, _i64, _int, _int, _p, _p, _p, _p, _sz, _p]),
    "spt_cross_entropy_workspace_bytes": (_sz, [_i64]),
    "spt_cross_entropy_fwd_f32": (_int, [_p, _p, _i64, _int, _i64, _p, _p, _p, _p, _sz, _p]),
    "spt_cross_entropy_bwd_f32": (_int, [_p, _p, _p, _i64, _int, _i64, _p, _p, _p, _p]),
    "spt_hist_loss_fwd_f32": (_int, [_p, _p, _i64, _int, _int, _int, _i64, _p, _p, _p, _p, _p, _sz, _p]),
    "spt_hist_loss_bwd_f32": (_int, [_p, _p, _i64, _int, _int, _int, _i64, _p, _p, _p, _p, _p]),
    "spt_confusion_matrix_i64": (_int, [_p, _p, _i64, _int, _int, _p, _p]),
    "spt_skinny_dw_supported": (_int, [_int, _int]),
    "spt_skinny_dw_workspace_bytes": (_sz, [_int, _int]),
    "spt_skinny_dw_f32": (_int, [_p, _p, _i64, _int, _int, _p, _p, _p, _sz, _p]),
    "spt_skinny_linear_f32": (_int, [_p, _i64, _int, _p, _p, _int, _p, _p]),
    "spt_skinny_linear_wt_f32": (_int, [_p, _i64, _int, _p, _int, _p, _p]),
    "spt_skinny_pre_supported": (_int, [_int, _int, _int]),
    "spt_skinny_linear_pre_f32": (_int, [_p, _i64, _int, _p, _p, _int, _p, _p, _p, _p, _p, _int, _p, _p]),
    "spt_skinny_dw_pre_f32": (_int, [_p, _p, _i64, _int, _int, _p, _p, _p, _p, _p, _p, _int, _p, _sz, _p]),
    "spt_skinny_use_split_bf16": (_int, [_int]),
    "spt_skinny_linear_pre_m_f32": (_int, [_p, _i64, _int, _p, _p, _int, _p, _p, _p, _p, _p, _int, _p, _int, _p]),
    "spt_skinny_linear_wt_m_f32": (_int, [_p, _i64, _int, _p, _int, _p, _int, _p]),
    "spt_skinny_dw_pre_m_f32": (_int, [_p, _p, _i64, _int, _int, _p, _p, _p, _p, _p, _p, _int, _int, _p, _sz, _p]),
    "spt_skinny_linear_bwd_supported": (_int, [_int, _int, _int, _int]),
    "spt_skinny_linear_bwd_workspace_bytes": (_sz, [_int, _int]),
    "spt_skinny_linear_bwd_m_f32": (_int, [_p, _p, _p, _i64, _int, _int, _p, _p, _p, _p, _p, _p, _p, _int, _int,
                                           _p, _sz, _p]),
    "spt_skinny_bwd_fused": (_int, [_int]),
    "spt_index_inverse": (_int, [_p, _i64, _i64, _p, _p]),
    "spt_select_edges_workspace_bytes": (_sz, [_i64]),
    "spt_select_edges": (_int, [_p, _i64, _i64, _p, _i64, _p, _i64, _p, _p, _p, _sz, _p]),
    "spt_cluster_select_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "spt_cluster_select": (_int, [_p, _p, _i64, _p, _i64, _i64, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "spt_relabel_consecutive_workspace_bytes": (_sz, [_i64]),
    "spt_relabel_consecutive": (_int, [_p, _p, _i64, _i64, _p, _p, _p, _p, _sz, _p]),
    "spt_radius_ball_workspace_bytes": (_sz, [_i64]),
    "spt_radius_ball_f32": (_int, [_p, _i64, _p, _f32, _int, _p, _i64, _p, _p, _p, _sz, _p]),
    "spt_cluster_pair_anchors_f32": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _int, _int, _p, _p, _p]),
    "spt_adjacency_stats_workspace_bytes": (_sz, [_i64]),
    "spt_adjacency_stats": (_int, [_p, _p, _i64, _i64, _int, _p, _p, _p, _sz, _p]),
    "spt_adjacency_regression": (_int, [_p, _p, _p, _i64, _i64, _int, _f32, _f32, _p, _p, _sz, _p]),
    "spt_adjacency_count_workspace_bytes": (_sz, [_i64]),
    "spt_adjacency_count": (_int, [_p, _i64, _i64, _int, _p, _p, _p, _i64, _int, _p, _p, _p, _sz, _p]),
    "spt_adjacency_fill_workspace_bytes": (_sz, [_i64, _i64]),
    "spt_adjacency_fill": (_int, [_p, _p, _i64, _i64, _int, _f32, _f32, _p, _p, _p, _p, _i64, _int, _int,
                                  _p, _p, _i64, _p, _p, _p, _p, _sz, _p]),
    "spt_ground_bounds_workspace_bytes": (_sz, [_i64]),
    "spt_ground_bounds_f32": (_int, [_p, _i64, _f32, _p, _p, _sz, _p]),
    "spt_ground_cell_min_f32": (_int, [_p, _i64, _f32, _i64, _i64, _i64, _i64, _p, _p]),
    "spt_ground_trim_workspace_bytes": (_sz, [_i64]),
    "spt_ground_trim_f32": (_int, [_p, _i64, _p, _int, _f32, _p, _f32, _p, _i64, _p, _i64, _p, _p, _sz, _p]),
    "spt_ground_ransac_workspace_bytes": (_sz, [_int]),
    "spt_ground_ransac_f32": (_int, [_p, _i64, _p, _p, _i64, _p, _p, _int, _f64, _p, _p, _p, _sz, _p]),
    "spt_ground_elevation_f32": (_int, [_p, _i64, _p, _f32, _p, _p]),
    "spt_point_color_workspace_bytes": (_sz, [_i64]),
    "spt_point_color_f32": (_int, [_p, _int, _i64, _int, _p, _i64, _p, _i64, _p, _i64, _p, _sz, _p]),
    "spt_point_density_f32": (_int, [_p, _i64, _p, _i64, _i64, _int, _p, _p]),
    "spt_augment_features_f32": (_int, [_p, _p, _i64, _int, _i64, _i64, _int, _c.c_uint64, _f64, _f64,
                                        _f64, _f64, _c.c_uint64, _c.c_uint64, _f32, _p]),
    "spt_augment_geometry_f32": (_int, [_p, _p, _i64, _i64, _i64, _int, _int, _c.c_uint64, _f64, _f64,
                                        _f64, _f64, _p, _p, _f32, _int, _p]),
    "spt_augment_color_range_f32": (_int, [_p, _i64, _i64, _int, _c.c_uint64, _f64, _f64, _f64, _f64,
                                           _p, _p]),
    "spt_augment_color_f32": (_int, [_p, _p, _i64, _i64, _i64, _int, _c.c_uint64, _f64, _f64, _f64,
                                     _f64, _p, _f32, _f32, _p]),
    "spt_voxel_bounds_f32": (_int, [_p, _i64, _i64, _f32, _p, _p, _p]),
    "spt_voxel_groups_workspace_bytes": (_sz, [_i64, _int]),
    "spt_voxel_groups_f32": (_int, [_p, _i64, _i64, _f32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz,
                                    _p]),
    "spt_voxel_mean_f32": (_int, [_p, _i64, _int, _i64, _p, _p, _i64, _int, _p, _i64, _p]),
    "spt_voxel_hist_i64": (_int, [_p, _i64, _p, _p, _i64, _int, _p, _p, _p, _p]),
    "spt_voxel_last": (_int, [_p, _p, _i64, _i64, _c.c_uint64, _int, _p, _p]),
    "spt_row_argmax_f32": (_int, [_p, _i64, _int, _p, _int, _p, _p, _p]),
    "spt_rows_accumulate_f32": (_int, [_p, _i64, _p, _p, _i64, _int, _p, _int, _p, _p]),
    "spt_labels_by_index_i64": (_int, [_p, _i64, _p, _i64, _p, _i64, _p, _p, _p, _int, _p, _p, _p]),
    "spt_labels_by_cluster_i64": (_int, [_p, _i64, _p, _p, _p, _i64, _i64, _p, _p, _int, _p, _p, _p]),
    "spt_instance_extents_i64": (_int, [_p, _i64, _p, _i64, _p, _p]),
    "spt_merge_instances_workspace_bytes": (_sz, [_i64, _int]),
    "spt_merge_instances_i64": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _int, _p, _p, _p, _p,
                                       _p, _p, _sz, _p]),
    "spt_pair_stats_workspace_bytes": (_sz, [_i64, _i64, _int]),
    "spt_pair_stats_i64": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _int, _i64, _int, _p, _p, _p, _p, _p,
                                  _p, _p, _p, _p, _p, _sz, _p]),
    "spt_panoptic_counts_workspace_bytes": (_sz, [_int]),
    "spt_panoptic_counts_i64": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _int, _p, _p, _p,
                                       _sz, _p]),
    "spt_weighted_group_mean_workspace_bytes": (_sz, [_i64, _i64]),
    "spt_weighted_group_mean_f32": (_int, [_p, _i64, _int, _p, _p, _i64, _p, _p, _p, _sz, _p]),
    "spt_instance_major_workspace_bytes": (_sz, [_i64]),
    "spt_instance_major_i64": (_int, [_p, _p, _p, _p, _i64, _i64, _int, _p, _p, _p, _p, _p, _sz, _p]),
    "spt_edge_affinity_loss_workspace_bytes": (_sz, [_i64]),
    "spt_edge_affinity_loss_fwd_f32": (_int, [_p, _p, _p, _i64, _p, _p, _p, _i64, _p, _p, _p, _p, _p, _p,
                                              _p, _sz, _p]),
    "spt_edge_affinity_loss_bwd_f32": (_int, [_p, _p, _p, _i64, _p, _p, _p, _i64, _p, _p, _p, _p, _p, _p]),
    "spt_partition_loss_workspace_bytes": (_sz, [_i64, _i64]),
    "spt_partition_loss_fwd_f32": (_int, [_p, _i64, _i64, _int, _p, _int, _int, _p, _i64, _f64, _f64, _f64,
                                          _f64, _f64, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "spt_partition_loss_bwd_f32": (_int, [_p, _i64, _i64, _int, _p, _i64, _p, _p, _p, _p, _p, _f64, _f64,
                                          _f64, _f64, _p, _p, _p, _i64, _p]),
    "spt_superedge_capacity": (_int, []),
    "spt_superedge_workspace_bytes": (_sz, [_i64]),
    "spt_superedge_classify": (_int, [_p, _i64, _p, _i64, _i64, _p, _p, _p, _sz, _p]),
    "spt_superedge_pair_offsets": (_int, [_p, _i64, _p, _p, _sz, _p]),
    "spt_superedge_f32": (_int, [_p, _i64, _p, _p, _i64, _p, _i64, _i64, _p, _p, _i64, _i64, _f32, _int,
                                 _f32, _int, _int, _p, _p, _p, _p, _p, _i64, _p]),
    "spt_component_graph_workspace_bytes": (_sz, [_i64]),
    "spt_component_graph_f32": (_int, [_p, _i64, _i64, _p, _p, _i64, _i64, _int, _p, _i64, _p, _p, _p,
                                       _sz, _p]),
    "spt_merge_means_f64": (_int, [_p, _p, _i64, _int, _p, _p]),
    "spt_merge_choose_f64": (_int, [_p, _p, _i64, _int, _p, _i64, _i64, _p, _f64, _p, _p, _p]),
    "spt_merge_resolve": (_int, [_p, _p, _i64, _i64, _int, _p, _p, _p]),
    "spt_merge_jump": (_int, [_p, _i64, _p, _p, _p]),
    "spt_merge_accumulate_workspace_bytes": (_sz, [_i64, _i64]),
    "spt_merge_accumulate_f64": (_int, [_p, _i64, _i64, _p, _p, _int, _p, _p, _p, _p, _p, _sz, _p]),
    "spt_edge_weights_workspace_bytes": (_sz, [_i64]),
    "spt_edge_weights_f32": (_int, [_p, _i64, _int, _i64, _p, _i64, _i64, _p, _p, _p, _p, _sz, _p]),
    "spt_sparse_bounds_i32": (_int, [_p, _p, _i64, _p, _p]),
    "spt_sparse_map_count_workspace_bytes": (_sz, [_i64, _int]),
    "spt_sparse_map_count": (_int, [_p, _p, _i64, _p, _p, _int, _int, _p, _p, _p, _p, _p, _sz, _p]),
    "spt_sparse_map_fill": (_int, [_p, _p, _i64, _p, _p, _int, _int, _p, _p, _p, _i64, _p, _p, _p, _p]),
    "spt_sparse_map_by_offset_workspace_bytes": (_sz, [_i64]),
    "spt_sparse_map_by_offset": (_int, [_p, _i64, _int, _p, _p, _p, _sz, _p]),
    "spt_sparse_conv_supported": (_int, [_int, _int]),
    "spt_sparse_conv_fwd_f32": (_int, [_p, _i64, _int, _p, _int, _int, _p, _p, _p, _p, _int, _p, _p]),
    "spt_sparse_conv_dw_workspace_bytes": (_sz, [_int, _int, _int]),
    "spt_sparse_conv_dw_f32": (_int, [_p, _p, _i64, _int, _int, _int, _p, _p, _p, _p, _i64, _p, _p, _sz, _p]),
    "spt_sparse_conv_dbias_workspace_bytes": (_sz, [_int]),
    "spt_sparse_conv_dbias_f32": (_int, [_p, _i64, _int, _p, _p, _sz, _p]),
}


class GnFwdTables(ctypes.Structure):
    """``spt_gn_fwd_tables`` of include/spt_hip.h (host struct of device pointers)."""
    _fields_ = [("weight", _p), ("mean_scale", _p), ("eps", _f32), ("mean", _p), ("rstd", _p),
                ("am", _p), ("scale", _p)]


class GnBwdTables(ctypes.Structure):
    """``spt_gn_bwd_tables`` of include/spt_hip.h."""
    _fields_ = [("weight", _p), ("mean_scale", _p), ("mean", _p), ("rstd", _p), ("c1", _p), ("c2", _p),
                ("c3", _p), ("gweight", _p), ("gbias", _p), ("gmean_scale", _p)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (hipcc --offload-arch=gfx950). There is no fallback path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a symbol
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def last_error():
    return lib.spt_last_error().decode("utf-8", "replace")


def check(status, what):
    if status != 0:
        raise RuntimeError(f"{what} failed ({status}): {last_error()}")


def ptr(t):
    """Device pointer of a tensor (or None)."""
    return None if t is None else t.data_ptr()


def dense(t, dtype=None, align=16):
    """``t`` as the kernels' contract wants it (include/spt_hip.h: row-major, contiguous, of the
    entry's element type, base address a multiple of ``align`` bytes), or None for None.

    The SAME tensor object comes back when it already is all of that - the hot path hands over
    fresh dense tensors and pays three attribute reads; anything else (a column slice, a strided
    or transposed or expanded view, another dtype, a dense view that starts 4 or 8 bytes into a
    16-byte line - a flat-buffer view, a row-narrowed view of rows that are no multiple of 16 bytes)
    becomes one dense copy, which comes from the allocator and is therefore aligned.  Every
    wrapper normalises its inputs and its incoming gradients through here: the kernels take raw
    pointers and index them by shape alone."""
    if t is None:
        return None
    if dtype is not None and t.dtype != dtype:
        return t.to(dtype, memory_format=torch.contiguous_format)      # cast and layout in one copy
    if not t.is_contiguous():
        return t.contiguous()
    if t.data_ptr() % align:
        return t.clone()
    return t


def stream_ptr(device=None):
    """hipStream_t of torch's current stream, as an integer."""
    return torch.cuda.current_stream(device).cuda_stream


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "superpoint_transformer_amd ops run on the MI355X only: got a "
                f"{t.device} tensor (no CPU fallback is provided)")
