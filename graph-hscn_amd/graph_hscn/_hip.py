"""ctypes binding of the C ABI in include/hscn.h (libhscn.so, gfx950).

The product path has no CPU or eager-PyTorch fallback: every operator in
``graph_hscn.nn`` goes through this library, and using one without it (or on a
CPU tensor) raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p
from typing import Optional

import torch

# HSCN_LIB: alternative build of the same ABI (the stamped diagnostic build used by tools/diag_resident.py)
_LIB_PATH = os.environ.get("HSCN_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libhscn.so")
_lib: Optional[ctypes.CDLL] = None

ABI_VERSION = 24
# `flags` of the resident entry points (include/hscn.h)
STORE_F16 = 1
GRAD_ACCUMULATE = 2
ACT = {"identity": 0, "relu": 1, "elu": 2, "tanh": 3}

P = c_void_p
_SIGNATURES = {
    # name: (restype, argtypes)
    "hscn_abi_version": (c_int, []),
    "hscn_strerror": (c_char_p, [c_int]),
    "hscn_csr_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "hscn_csr_build": (c_int, [P, P, c_int64, c_int64, c_int64, P, P, P, P, P, c_size_t, P]),
    "hscn_csr_pair_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "hscn_csr_build_pair": (c_int, [P, P, c_int64, c_int64, c_int64, P, P, P, P, P, P, P, P, c_size_t, P]),
    "hscn_csr_cross_positions": (c_int, [P, P, c_int64, P, P, P]),
    "hscn_gcn_dinv": (c_int, [P, c_int64, P, P]),
    "hscn_gcn_norm_weights": (c_int, [P, P, P, P, c_int64, P, P, P]),
    "hscn_linear_fwd": (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int, c_int, c_int, c_int, P]),
    "hscn_linear_bwd_w_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "hscn_linear_bwd_w": (c_int, [P, P, P, P, c_int64, c_int, c_int, c_int, P, c_size_t, P]),
    "hscn_act_fwd": (c_int, [P, P, c_int64, c_int, P]),
    "hscn_act_bwd": (c_int, [P, P, P, c_int64, c_int, P]),
    "hscn_dropout": (c_int, [P, P, c_int64, c_float, c_uint64, P]),
    "hscn_spmm_csr_gcn": (c_int, [P, P, P, P, P, P, P, c_int64, c_int, c_int, c_int, P]),
    "hscn_spmm_csr_weighted": (c_int, [P, P, P, P, P, P, c_int64, c_int, P]),
    "hscn_gat_segment_fwd": (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int, c_float, c_int, c_int, P]),
    "hscn_gat_segment_bwd_dst": (c_int, [P, P, P, P, P, P, P, P, P, c_int64, c_int, c_float, P]),
    "hscn_gat_segment_bwd_src": (c_int, [P, P, P, P, P, P, P, P, P, c_int64, c_int, P]),
    "hscn_segment_mean_fwd": (c_int, [P, P, P, P, c_int64, c_int, P]),
    "hscn_segment_mean_bwd": (c_int, [P, P, P, P, c_int64, c_int, P]),
    "hscn_mincut_sparse_fwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, c_int, P]),
    "hscn_mincut_sparse_bwd": (c_int, [P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, P]),
    "hscn_dmon_sparse_fwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, c_int, P]),
    "hscn_dmon_sparse_bwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, P]),
    "hscn_bgemm_f32": (c_int, [P, P, P, c_int64, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int64, c_int64,
                               c_int64, c_int, P]),
    "hscn_mincut_dense_fwd": (c_int, [P, P, P, c_int64, c_int, c_int, c_int, P, P, P, P, P, P, P, P, P]),
    "hscn_mincut_dense_bwd": (c_int, [P, P, P, P, P, P, P, c_int64, c_int, c_int, P, P, P, P, P]),
    "hscn_assign_argmax": (c_int, [P, P, c_int64, c_int, P]),
    "hscn_to_dense_adj": (c_int, [P, P, c_int64, c_int64, P, P]),
    "hscn_to_dense_adj_batched": (c_int, [P, P, c_int64, c_int64, c_int64, P, P]),
    "hscn_build_hetero_count": (c_int, [P, c_int, P, P, c_int64, c_int, c_int, P, P, P, P, P]),
    "hscn_build_hetero_scan": (c_int, [P, c_int64, P, P, P, P, P, P, P]),
    "hscn_build_hetero_emit": (c_int, [P, P, P, P, P, P, c_int64, c_int, c_int, c_int64, c_int64, P, P, P, P, P]),
    "hscn_collate_gather": (c_int, [P, P, c_int64, P, P, P, P, P]),
    "hscn_criterion_fwd": (c_int, [P, P, c_int64, c_int, P, P, P, P]),
    "hscn_scale": (c_int, [P, P, P, c_int64, P]),
    "hscn_scn_resident_supported": (c_int, [c_int] * 5),
    "hscn_scn_resident_param_count": (c_int64, [c_int] * 3),
    "hscn_scn_resident_fwd": (c_int, [P, P, c_int64, P, P, c_int64, c_int64, c_int, c_int, c_int, c_int, P, P, P, P, P,
                                      c_int, c_int, P, P, P, P, P, P, P, P, P, P, P, P, P, c_int, P]),
    "hscn_scn_resident_bwd": (c_int, [P, P, c_int64, P, P, c_int64, c_int64, c_int, c_int, c_int, c_int, P, P, P, P, P,
                                      P, P, P, P, P, P, P, P, c_int, c_int, P, P, P, c_int, P]),
    "hscn_scn_resident_train_step_supported": (c_int, [c_int] * 5),
    "hscn_scn_resident_train_step": (c_int, [P, P, c_int64, P, P, c_int64, c_int64, c_int, c_int, c_int, c_int, P, P, P,
                                             P, P, P, P, c_int, c_int, P, P, P, P, P, P, P, P, P, c_int, P]),
    "hscn_scn_resident_train_epoch": (c_int, [P, P, P, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int, P, P, P, P, P,
                                              P, P, c_int, c_int, P, P, P, P, P, P, P, c_int, P]),
    "hscn_adam_step": (c_int, [P, P, c_int, P, P, P, c_int64, P, P, P, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                               ctypes.c_double, c_int, P]),
    "hscn_adam_step_ex": (c_int, [P, P, c_int, P, P, P, c_int64, P, P, P, ctypes.c_double, ctypes.c_double,
                                  ctypes.c_double, ctypes.c_double, c_int, c_float, P, c_int, P]),
    "hscn_clip_grad_norm_flat": (c_int, [P, c_int64, c_float, P, P]),
    "hscn_resident_supported": (c_int, [c_int] * 8),
    "hscn_resident_launch_plan": (c_int, [c_int] * 9 + [P]),
    "hscn_resident_launch_plan_ex": (c_int, [c_int] * 10 + [P]),
    "hscn_resident_param_count": (c_int64, [c_int] * 4),
    "hscn_resident_fwd": (c_int, [P, P, P, c_int64, P, c_int64, P, c_int64, P, P, P, P, P, c_int64, c_int64,
                                  c_int64, c_int, c_int, c_int, c_int, c_int, c_float, P, P, P, P, P, c_int,
                                  c_int, c_int, c_int, c_int, P, P, P, P, P, P, P, P, P, P, c_int, P]),
    "hscn_resident_bwd": (c_int, [P, P, c_int64, P, P, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, P,
                                  P, P, P, P, P, P, P, P, P, P, c_int, c_int, P, P, P, P, c_int, P]),
    "hscn_resident_fwd_with_virtual": (c_int, [P, P, c_int64, P, P, c_int64, c_int64, c_int, c_int, c_int, c_int,
                                               c_int, P, P, P, P, P, c_int, c_int, P, P, P, P, P, P, P, P, P, P, c_int,
                                               P]),
    "hscn_resident_bwd_with_virtual": (c_int, [P, P, c_int64, P, P, c_int64, c_int64, c_int, c_int, c_int, c_int,
                                               c_int, P, P, P, P, P, P, P, P, P, P, P, c_int, c_int, P, P, P, P, P,
                                               c_int, P]),
    "hscn_resident_train_step_supported": (c_int, [c_int] * 8),
    "hscn_resident_train_step_wgs_per_cu": (c_int, [c_int] * 8),
    "hscn_resident_train_step": (c_int, [P, P, c_int64, P, P, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, P,
                                         P, P, P, P, c_int, c_int, P, c_int, P, P, P, P, P, P, P, P, P, c_int, P]),
    "hscn_resident_structure": (c_int, [P, c_int64, P, c_int64, P, c_int64, P, P, P, P, P, c_int64, c_int, c_int, c_int,
                                        c_int, P, P, P]),
    "hscn_collate_gather_structure": (c_int, [P, P, P, c_int64, P, P, P, P, P, P]),
    "hscn_mincut_dense_ragged_fwd": (c_int, [P, P, c_int, P, P, c_int64, c_int64, c_int, c_int, c_int, P, P, P, P, P, P, P, P, P]),
    "hscn_mincut_dense_ragged_bwd": (c_int, [P, c_int, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, c_int, P, P, P, P, P]),
    "hscn_dense_adj_s": (c_int, [P, c_int, P, P, c_int64, c_int, c_int, c_int, P, P, P]),
    "hscn_dense_adj_asymmetry_u8": (c_int, [P, c_int64, c_int, P, P]),
    "hscn_mincut_dense_ragged_bwd_sym": (c_int, [P, c_int, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, c_int, P, P, P, P, P, P]),
    "hscn_to_dense_adj_ragged_u8": (c_int, [P, P, c_int64, P, P, c_int64, c_int64, c_int64, c_int, P, P, P]),
    "hscn_to_dense_adj_ragged": (c_int, [P, P, c_int64, P, P, c_int64, c_int64, c_int64, c_int, P, P]),
    "hscn_gcn_norm_self_loops": (c_int, [P, P, P, c_int64, c_int64, c_float, P, P, P, P]),
    "hscn_norm_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "hscn_layer_norm_fwd": (c_int, [P, P, P, P, P, P, c_int64, c_int, c_float, P]),
    "hscn_layer_norm_bwd": (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int, P, c_size_t, P]),
    "hscn_batch_norm_fwd": (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int, c_float, c_float, c_int, P, c_size_t, P]),
    "hscn_batch_norm_bwd": (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int, c_int, P, c_size_t, P]),
    "hscn_comm_alloc": (c_int, [c_size_t, c_int, P]),
    "hscn_comm_free": (c_int, [P]),
    "hscn_comm_ipc_export": (c_int, [P, P]),
    "hscn_comm_ipc_open": (c_int, [P, P]),
    "hscn_comm_ipc_close": (c_int, [P]),
    "hscn_allreduce_oneshot_slot_bytes": (c_size_t, [c_int64, c_int]),
    "hscn_allreduce_oneshot_flag_bytes": (c_size_t, [c_int64, c_int]),
    "hscn_allreduce_oneshot_chunks": (c_int64, [c_int64]),
    "hscn_allreduce_oneshot": (c_int, [P, c_int64, P, P, P, P, c_int, c_int, c_float, ctypes.c_uint32, P]),
    # ABI 20: the MPNN baseline's one-launch step and forward (include/hscn.h)
    "hscn_mpnn_supported": (c_int, [c_int] * 6),
    "hscn_mpnn_param_count": (c_int64, [c_int] * 4),
    "hscn_mpnn_train_step": (c_int, [P, P, c_int64, P, P, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, P, c_int,
                                     c_int, P, c_int, c_float, P, P, P, P, P, c_float, c_uint64, P, c_int, P]),
    "hscn_mpnn_forward": (c_int, [P, P, c_int64, P, P, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, P, c_int,
                                  c_int, P, c_int, c_float, P, P, P, P, P, P]),
    # ABI 21: GATConv with the implicit self loop, narrow-row kernels (csrc/gat_loops.hip)
    "hscn_gat_loop_fwd": (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int, c_float, c_int, P]),
    "hscn_gat_loop_bwd_dst": (c_int, [P, P, P, P, P, P, P, P, P, c_int64, c_int, c_float, P]),
    "hscn_gat_loop_bwd_src": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int, c_float, P]),
    # ABI 22: the SignNet node encoder's forward as one launch (csrc/signnet.hip)
    "hscn_signnet_supported": (c_int, [c_int] * 12),
    "hscn_signnet_encode": (c_int, [P, P, P, c_int64, P, P, c_int64, c_int64] + [c_int] * 9 + [P, c_int, c_int, P, P,
                                    P, P]),
    # epoch metrics on the device (csrc/metrics.hip; additive to ABI 23)
    "hscn_average_precision_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "hscn_average_precision": (c_int, [P, P, c_int64, c_int, P, P, P, P, P, c_size_t, P]),
    "hscn_mean_absolute_error": (c_int, [P, P, c_int64, c_int, P, P, P]),
    # Laplacian PE statistics of a batch as one launch (csrc/lap_eig.hip; additive to ABI 23)
    "hscn_lap_eig_supported": (c_int, [c_int, c_int]),
    "hscn_lap_eig_lds_max_n": (c_int, []),
    "hscn_lap_eig_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "hscn_lap_eig_stats": (c_int, [P, c_int64, P, P, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, P, P, P, P,
                                   c_size_t, P]),
    # HSCN with the virtual -> local relation as one launch (csrc/resident_vl.hip; additive to ABI 23)
    "hscn_vl_supported": (c_int, [c_int] * 8),
    "hscn_vl_param_count": (c_int64, [c_int] * 4),
    "hscn_vl_train_step": (c_int, [P, P, P, c_int64, P, c_int64, P, c_int64, P, P, P, P, P, c_int64, c_int64, c_int64,
                                   c_int, c_int, c_int, c_int, c_int, c_float, P, P, P, P, P, c_int, c_int, c_int, c_int,
                                   P, c_int, c_float, P, P, P, P, P, P, c_int, P]),
    # schedules inside the optimizer launch and the one-launch Adagrad (csrc/optim.hip; additive to ABI 23);
    # `sched`: ctypes.byref(LRScheduleC) or None
    "hscn_adam_step_sched": (c_int, [P, P, c_int, P, P, P, c_int64, P, P, P, ctypes.c_double, ctypes.c_double,
                                     ctypes.c_double, ctypes.c_double, c_int, c_float, P, c_int, P, P, P]),
    "hscn_adagrad_step": (c_int, [P, P, c_int, P, P, c_int64, P, P, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                  c_float, P, c_int, P, P, P]),
    # class-index targets: fused log-softmax + NLL, accuracy / macro-F1 (csrc/loss.hip, csrc/metrics.hip; additive
    # to ABI 23)
    "hscn_softmax_nll_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "hscn_softmax_nll_fwd": (c_int, [P, P, c_int64, c_int, P, P, P, P, P, c_size_t, P]),
    "hscn_multiclass_metrics": (c_int, [P, P, c_int64, c_int, P, P, P, P, P]),
    # class weights / ignore_index of the multiclass criterion and the per-node head (csrc/loss.hip,
    # csrc/node_head.hip; additive to ABI 23)
    "hscn_class_weights": (c_int, [P, c_int64, c_int, c_int64, c_int, P, P, P, P, P, P]),
    "hscn_softmax_nll_fwd_ex": (c_int, [P, P, c_int64, c_int, P, c_int64, P, P, P, P, P, P, c_size_t, P]),
    "hscn_node_head_supported": (c_int, [c_int, c_int]),
    "hscn_node_head_rows_per_workgroup": (c_int, []),
    "hscn_node_head_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "hscn_node_head_fwd": (c_int, [P, P, P, P, P, c_int64, c_int, c_int, c_int, P, P]),
    "hscn_node_head_bwd": (c_int, [P, P, P, P, P, P, P, c_int64, c_int, c_int, c_int, P, P, P, P, P, c_int, P,
                                   c_size_t, P]),
    # link-level tasks: the pair decoder and the per-graph ranking metric (csrc/edge_head.hip; additive to ABI 23)
    "hscn_pair_dot_supported": (c_int, [c_int]),
    "hscn_pair_dot_pairs_per_workgroup": (c_int, [c_int]),
    "hscn_pair_dot_fwd": (c_int, [P, P, c_int64, c_int64, c_int, P, P, P]),
    "hscn_pair_dot_bwd": (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, P, P]),
    "hscn_pair_rank_supported": (c_int, [c_int, c_int]),
    "hscn_pair_rank_lds_max_nodes": (c_int, [c_int]),
    "hscn_pair_rank_max_workgroups": (c_int, []),
    "hscn_pair_rank": (c_int, [P, P, P, P, P, P, P, c_int64, c_int64, c_int64, c_int, c_int, c_int, P, P, P, P]),
    "hscn_pair_rank_reduce": (c_int, [P, c_int64, c_int, P, P, P, P, P]),
    "hscn_vl_forward": (c_int, [P, P, P, c_int64, P, c_int64, P, c_int64, P, P, P, P, P, c_int64, c_int64, c_int64,
                                c_int, c_int, c_int, c_int, c_int, c_float, P, P, P, P, P, c_int, c_int, c_int, c_int,
                                P, c_int, c_float, P, P, P, P, P, P, P]),
    # random-walk structural encoding of a batch as one launch (csrc/rwse.hip; additive to ABI 23)
    "hscn_rwse_supported": (c_int, [c_int, c_int]),
    "hscn_rwse_tile": (c_int, []),
    "hscn_rwse_stats": (c_int, [P, P, P, c_int64, c_int64, c_int, c_int, P, P, P]),
    # GINEConv's aggregate with edge features (csrc/gine.hip; additive to ABI 23)
    "hscn_gine_supported": (c_int, [c_int, c_int]),
    "hscn_gine_long_row": (c_int, []),
    "hscn_gine_chunk": (c_int, []),
    "hscn_gine_aggregate_fwd": (c_int, [P, P, P, P, P, P, P, c_float, P, c_int64, c_int64, c_int, c_int, P, P]),
    "hscn_gine_aggregate_bwd_x": (c_int, [P, P, P, P, P, P, P, c_float, P, P, c_int64, c_int64, c_int, c_int, P, P]),
    "hscn_gine_aggregate_bwd_msg": (c_int, [P, P, P, P, P, P, P, c_int64, c_int64, c_int, c_int, P, P]),
    # global attention: block-diagonal multi-head self-attention (csrc/attention.hip; additive to ABI 24)
    "hscn_attention_supported": (c_int, [c_int, c_int]),
    "hscn_attention_tile": (c_int, []),
    "hscn_attention_chunk": (c_int, []),
    "hscn_attention_fwd": (c_int, [P, P, c_int64, c_int64, c_int, c_int, c_int, P, P, P, P]),
    "hscn_attention_bwd_q": (c_int, [P, P, P, P, P, c_int64, c_int64, c_int, c_int, c_int, P, P, P, P]),
    "hscn_attention_bwd_kv": (c_int, [P, P, P, P, P, c_int64, c_int64, c_int, c_int, c_int, P, P, P]),
    # GatedGCN's aggregate: edge-gated sums, edge features in and out (csrc/gatedgcn.hip; additive to ABI 24)
    "hscn_gatedgcn_supported": (c_int, [c_int]),
    "hscn_gatedgcn_long_row": (c_int, []),
    "hscn_gatedgcn_chunk": (c_int, []),
    "hscn_gatedgcn_fwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, P, P]),
    "hscn_gatedgcn_bwd_dst": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, P, P]),
    "hscn_gatedgcn_bwd_src": (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, P, P]),
    # categorical encoders: gather-sum, stable counting sort, long-row segment reduce (csrc/catenc.hip; additive to
    # ABI 24); `card_host`: a host array of F int32 (host_cards)
    "hscn_catenc_supported": (c_int, [c_int, c_int, c_int]),
    "hscn_catenc_long_row": (c_int, []),
    "hscn_catenc_chunk": (c_int, []),
    "hscn_catenc_sort_chunk": (c_int, []),
    "hscn_catenc_fwd": (c_int, [P, P, P, P, c_int64, c_int, c_int, P, P]),
    "hscn_catenc_index_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "hscn_catenc_index_build": (c_int, [P, P, c_int64, c_int, P, P, P, P, c_size_t, P]),
    "hscn_catenc_bwd_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "hscn_catenc_bwd": (c_int, [P, P, P, P, c_int64, c_int, c_int, c_int, P, P, c_size_t, P]),
    # edge attention: TransformerConv's multi-head softmax over in-edges (csrc/edge_attention.hip; additive to ABI 24)
    "hscn_edge_attn_supported": (c_int, [c_int, c_int]),
    "hscn_edge_attn_long_row": (c_int, []),
    "hscn_edge_attn_chunk": (c_int, []),
    "hscn_edge_attn_fwd": (c_int, [P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int64, c_int, c_int, P, P]),
    "hscn_edge_attn_bwd_dst": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int64, c_int, c_int,
                                       P, P]),
    "hscn_edge_attn_bwd_src": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int64, c_int, c_int,
                                       P, P]),
    # shortest-path buckets and the attention they bias (csrc/spd.hip, csrc/attention.hip; additive to ABI 24)
    "hscn_spd_supported": (c_int, [c_int, c_int]),
    "hscn_spd_buckets": (c_int, [P, P, P, P, c_int64, c_int64, c_int64, c_int64, c_int, c_int, P, P, P]),
    "hscn_attention_bias_supported": (c_int, [c_int, c_int, c_int]),
    "hscn_attention_bias_fwd": (c_int, [P, P, P, P, P, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int, P, P, P,
                                        P]),
    "hscn_attention_bias_bwd_q": (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int,
                                          P, P, P, P, c_int64, P, P]),
    "hscn_attention_bias_bwd_kv": (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int64, c_int64, c_int, c_int, c_int,
                                           c_int, P, P, P]),
    "hscn_expander_max_nodes": (c_int, []),
    "hscn_expander_max_degree": (c_int, []),
    "hscn_expander_build": (c_int, [P, P, c_int64, c_int64, c_int, c_uint64, c_int, P, P, P]),
    "hscn_exph_attn_supported": (c_int, [c_int, c_int]),
    "hscn_exph_attn_long_row": (c_int, []),
    "hscn_exph_attn_chunk": (c_int, []),
    "hscn_exph_type_long_row": (c_int, []),
    "hscn_exph_type_chunk": (c_int, []),
    "hscn_exph_max_types": (c_int, []),
    "hscn_exph_attn_fwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int64, c_int, c_int, c_int, P,
                                   P]),
    "hscn_exph_attn_bwd_dst": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int64, c_int,
                                       c_int, c_int, P, P]),
    "hscn_exph_attn_bwd_src": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int64, c_int,
                                       c_int, c_int, P, P]),
    "hscn_exph_type_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "hscn_exph_attn_bwd_type": (c_int, [P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, c_int, c_int, P, P,
                                        c_size_t, P]),
    # LapPE node encoder, DeepSet model: fused chain + masked sum over the frequencies (csrc/lappe.hip; additive to
    # ABI 24); `params_host`: a host array of 2 * layers device pointers (engine._ptr_table)
    "hscn_lappe_supported": (c_int, [c_int, c_int, c_int]),
    "hscn_lappe_tile": (c_int, []),
    "hscn_lappe_workspace_floats": (c_int64, [c_int64, c_int, c_int, c_int]),
    "hscn_lappe_fwd": (c_int, [P, P, P, c_int64, c_int, c_int, c_int, c_int, c_uint64, P, P]),
    "hscn_lappe_bwd": (c_int, [P, P, P, P, c_int64, c_int, c_int, c_int, c_int, c_uint64, P, P, c_int64, P]),
    # PNAConv's aggregate: mean / min / max / sum / std under degree scalers (csrc/pna.hip; additive to ABI 24);
    # `aggregators_host` / `scalers_host`: host arrays of int32 codes (nn.functional.PNA_AGGREGATORS / PNA_SCALERS)
    "hscn_pna_supported": (c_int, [c_int, c_int, c_int]),
    "hscn_pna_long_row": (c_int, []),
    "hscn_pna_chunk": (c_int, []),
    "hscn_pna_fwd": (c_int, [P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, P, c_int, P, c_int, c_float, P, P]),
    "hscn_pna_bwd_fold": (c_int, [P, P, P, P, P, c_int64, c_int, P, c_int, P, c_int, c_float, P]),
    "hscn_pna_bwd_src": (c_int, [P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, P, P]),
    "hscn_pna_bwd_edge": (c_int, [P, P, P, P, P, P, P, c_int64, c_int64, c_int, P, P]),
    # SAN's attention over real and fake edges (csrc/san.hip; additive to ABI 24)
    "hscn_san_attn_supported": (c_int, [c_int, c_int, c_int]),
    "hscn_san_attn_fwd": (c_int, [P] * 12 + [c_int64, c_int64, c_int64, c_int, c_int, c_int, ctypes.c_double, c_int, P,
                                            P]),
    "hscn_san_attn_bwd_dst": (c_int, [P] * 17 + [c_int64, c_int64, c_int64, c_int, c_int, c_int, ctypes.c_double, c_int,
                                                 P, P]),
    "hscn_san_attn_bwd_src": (c_int, [P] * 16 + [c_int64, c_int64, c_int64, c_int, c_int, c_int, ctypes.c_double, c_int,
                                                 P, P]),
    # GCNII's layer, PyG GCN2Conv: gather, mix, weight product and epilogue as one launch (csrc/gcn2.hip; additive to
    # ABI 24)
    "hscn_gcn2_supported": (c_int, [c_int]),
    "hscn_gcn2_plan": (c_int, [c_int, c_int, P]),
    "hscn_gcn2_fwd": (c_int, [P] * 9 + [c_int64, c_int, ctypes.c_double, ctypes.c_double, c_int, P]),
    "hscn_gcn2_bwd": (c_int, [P] * 7 + [c_int64, c_int, ctypes.c_double, ctypes.c_double, c_int, P]),
    "hscn_gcn2_bwd_w_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "hscn_gcn2_bwd_w": (c_int, [P] * 5 + [c_int64, c_int, ctypes.c_double, P, c_size_t, P]),
}


class LRScheduleC(ctypes.Structure):    # include/hscn.h: hscn_lr_schedule
    _fields_ = [("kind", c_int), ("base_lr", ctypes.c_double), ("warmup_steps", c_int64), ("total_steps", c_int64),
                ("period", c_int64), ("gamma", ctypes.c_double), ("min_factor", ctypes.c_double)]


class HipExtensionMissing(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Load libhscn.so once; fail loudly if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise HipExtensionMissing(
            f"{_LIB_PATH} not found: the graph_hscn operators run only through the gfx950 HIP "
            "library (build it with `make -C graph-hscn_amd` or __graft_entry__.build()); "
            "there is no CPU/eager fallback.")
    L = ctypes.CDLL(_LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(L, name)
        except AttributeError as e:  # pragma: no cover
            raise HipExtensionMissing(f"{_LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    v = L.hscn_abi_version()
    if v != ABI_VERSION:
        raise HipExtensionMissing(f"libhscn.so ABI {v} != expected {ABI_VERSION}")
    _lib = L
    return L


PLAN_FIELDS = ("threads", "db", "exp", "csr_launch", "two", "fwd_lds", "bwd_lds")      # include/hscn.h: HSCN_PLAN_*
# hscn_resident_launch_plan_ex: HSCN_LAUNCH_* in this order, and the fields it adds to the seven above
LAUNCHES = ("pair", "pair_virtual", "step", "step_virtual")
PLAN_FIELDS_EX = PLAN_FIELDS + ("csr_lds", "v_db", "v_exp", "v_acq", "bwd_v_db", "local_fixed", "virtual_fixed",
                                "fwd_local_need", "fwd_virtual_need", "bwd_local_need", "bwd_virtual_need")


def resident_launch_plan(F: int, H: int, L: int, C: int, max_n: int, max_v: int, max_ell: int, max_evv: int,
                         want_export: bool = True, launch: str = "pair") -> Optional[dict]:
    """What the graph-resident launches choose for these maxima (host arithmetic, no device needed), or None where
    the launch shape does not take them.  launch = "pair": hscn_resident_fwd / hscn_resident_bwd through
    hscn_resident_launch_plan, {"threads", "db", "exp", "csr_launch", "two", "fwd_lds", "bwd_lds"}.  Any other of
    LAUNCHES ("pair_virtual": the pair with virtual workgroups; "step" / "step_virtual": the one-launch step without /
    with a virtual job): every field of PLAN_FIELDS_EX through hscn_resident_launch_plan_ex."""
    if launch == "pair":
        buf = (ctypes.c_int32 * len(PLAN_FIELDS))()
        rc = lib().hscn_resident_launch_plan(F, H, L, C, max_n, max_v, max_ell, max_evv, int(bool(want_export)), buf)
        fields = PLAN_FIELDS
    else:
        rc, buf = resident_launch_plan_ex(LAUNCHES.index(launch), F, H, L, C, max_n, max_v, max_ell, max_evv, want_export)
        fields = PLAN_FIELDS_EX
    if rc == -3:
        return None
    check(rc, "hscn_resident_launch_plan")
    return dict(zip(fields, (int(v) for v in buf)))


def resident_launch_plan_ex(launch: int, F: int, H: int, L: int, C: int, max_n: int, max_v: int, max_ell: int,
                            max_evv: int, want_export: bool = True):
    """hscn_resident_launch_plan_ex as it is: (return code, the HSCN_PLAN_EX_COUNT fields; zeros unless the code is 0)."""
    buf = (ctypes.c_int32 * len(PLAN_FIELDS_EX))()
    rc = lib().hscn_resident_launch_plan_ex(launch, F, H, L, C, max_n, max_v, max_ell, max_evv, int(bool(want_export)),
                                            buf)
    return int(rc), [int(v) for v in buf]


def exported_symbols():
    return list(_SIGNATURES)


def ptr(t: Optional[torch.Tensor]):
    """Device pointer of a contiguous tensor (None -> NULL)."""
    if t is None:
        return None
    if hasattr(t, "materialize"):      # loss.LazyScaled reaching an operator that wants plain values
        t = t.materialize()
    if not t.is_cuda:
        raise RuntimeError(
            "graph_hscn operators take HIP device tensors only (got a CPU tensor): the hot path "
            "has no CPU fallback -- move the batch and model to 'cuda' (MI355X).")
    if not t.is_contiguous():
        raise RuntimeError("graph_hscn operators need contiguous tensors")
    return t.data_ptr()


def stream() -> int:
    """Raw handle of the current HIP stream of the current device (the private getter is ~20x cheaper than
    building a ``torch.cuda.Stream`` object; the eager path is host-bound)."""
    try:
        return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())
    except AttributeError:
        return torch.cuda.current_stream().cuda_stream


def check(rc: int, name: str) -> None:
    if rc != 0:
        msg = lib().hscn_strerror(rc)
        raise RuntimeError(f"{name} failed with code {rc}: {msg.decode() if msg else '?'}")


def call(name: str, *args) -> None:
    check(getattr(lib(), name)(*args), name)


class FlagWord:
    """One kernel family's flag word: per device a zero-initialised [1] int32 tensor that its launches OR bits into."""

    def __init__(self):
        self._words = {}

    def of(self, device) -> torch.Tensor:
        """The word of ``device`` (a device without an index is the current one)."""
        device = torch.device(device)
        if device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
        t = self._words.get(device)
        if t is None:
            t = self._words[device] = torch.zeros(1, dtype=torch.int32, device=device)
        return t

    def take(self, device) -> int:
        """Synchronising: read the word of ``device`` and clear it."""
        word = self.of(device)
        f = int(word.item())
        if f:
            word.zero_()
        return f
