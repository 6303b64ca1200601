"""ctypes binding of libsvr_hip.so (the C ABI declared in include/svr_hip.h).

There is NO fallback: if the library is missing this raises, and every op raises on a
non-GPU tensor.  (The CPU oracle lives under oracle/ and is test infrastructure only.)
"""
import ctypes as C
import os

import numpy as np
# torch is imported here, ahead of any CDLL in lib(): it must load ITS HIP runtime first.  libsvr_hip.so only names
# libamdhip64 by SONAME, and if the system copy gets mapped before torch's, the process ends up with two runtimes (kernels
# launched by one on memory owned by the other: "no ROCm-capable device" from rocPRIM).  stream() / ptr() / to_device() below
# need the module on every call, so it is not imported lazily.
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsvr_hip.so")

SVR_MAX_LEVELS = 6
EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_MASK = 0, 1, 2, 3

P = C.c_void_p
I32, I64, F32 = C.c_int32, C.c_int64, C.c_float


class Conv2dDesc(C.Structure):
    _fields_ = [("src0", P), ("src1", P), ("B", I32), ("H", I32), ("W", I32), ("C0", I32), ("C1", I32), ("k", I32),
                ("stride", I32), ("act", I32), ("upsample", I32)]


class Conv2dPlan(C.Structure):      # svr_conv2d_plan (tests/test_capi_cpu.py compares the layout with the header's)
    _fields_ = [(n, I32) for n in ("family", "vec4", "Ho", "Wo", "classes", "ksteps", "splits", "ksplit", "epilogue", "reduce_grid",
                                   "dy_vec4", "co", "kk", "grid", "capped", "rows_per_block", "parts", "ipg", "groups", "grid_y")] + \
               [(n, I64) for n in ("mtiles", "tiles", "split_stride", "rows_per_split", "last_rows", "workspace_bytes")]


class PullPlan(C.Structure):
    _fields_ = [("keys", P), ("recs", P), ("heads", P), ("n_items", I64)]


class Level(C.Structure):
    _fields_ = [("vol", P), ("gvol", P), ("C", I32), ("D", I32), ("H", I32), ("W", I32), ("col", I32), ("order", P),
                ("item_order", P), ("plan", C.POINTER(PullPlan))]


class GatherDesc(C.Structure):
    _fields_ = [("n_levels", I32), ("B", I32), ("N", I32), ("row_stride", I32), ("align_corners", I32),
                ("displacement", F32), ("order", P), ("level", Level * SVR_MAX_LEVELS), ("flags", I32)]


GATHER_WIDE_OFFSETS, GATHER_DETERMINISTIC = 1, 2
EVAL_SUMS_WORKSPACE_BYTES = 6144      # SVR_EVAL_SUMS_WORKSPACE_BYTES


# name -> (restype, argtypes): exactly the declarations of include/svr_hip.h
SIGNATURES = {
    "svr_version": (C.c_int, []),
    "svr_last_error": (C.c_char_p, []),
    "svr_sizeof_level": (I64, []),
    "svr_sizeof_gather_desc": (I64, []),
    "svr_points_morton_order_workspace": (I64, [I32, I32]),
    "svr_points_morton_order": (C.c_int, [P, P, P, I32, I32, P, P]),
    "svr_points_voxel_order": (C.c_int, [P, P, I32, I32, I32, I32, I32, I32, P, P]),
    "svr_gather_item_order": (C.c_int, [P, I32, I32, I32, I32, I32, I32, F32, I32, P, P, P]),
    "svr_gather_item_order_xblock": (C.c_int, [P, I32, I32, I32, I32, I32, I32, F32, I32, P, P, P]),
    "svr_gather_project_bwd": (C.c_int, [P, P, I64, I32, I32, I32, I32, I32, I32, F32, P, P, P]),
    "svr_gather_project_plan_workspace": (C.c_int64, [I32, I32]),
    "svr_gather_project_slots": (C.c_int64, [I32, I32, I32, I32, I32]),
    "svr_gather_project_plan": (C.c_int, [P, I32, I32, I32, I32, I32, I32, F32, P, P, P, P, P, P]),
    "svr_gather_project_bwd2": (C.c_int, [P, P, I64, I32, I32, I32, I32, I32, I32, F32, P, P, P, P, P, P]),
    "svr_gather_pull_plan_workspace": (I64, [I32, I32]),
    "svr_gather_pull_plan_workspace_cells": (I64, [I32, I32, I32, I32]),
    "svr_gather_pull_plan": (C.c_int, [P, I32, I32, I32, I32, I32, I32, I32, I32, I32, F32, P, P, P, P, P, P, P]),
    "svr_gather_trilinear_fwd": (C.c_int, [C.POINTER(GatherDesc), P, P, P]),
    "svr_gather_fc0_supported": (C.c_int32, [C.POINTER(GatherDesc)]),
    "svr_gather_fc0_workspace": (C.c_int64, [C.POINTER(GatherDesc), I32]),
    "svr_gather_fc0_fwd": (C.c_int, [C.POINTER(GatherDesc), P, P, I64, P, P, I64, I32, P, I64, P, C.c_uint32, I32, P, P]),
    "svr_gather_fc0_prepare": (C.c_int, [C.POINTER(GatherDesc), P, I64, I32, P, I64, P, C.c_uint32, P, P]),
    "svr_gather_fc0_run": (C.c_int, [C.POINTER(GatherDesc), P, P, P, I64, I32, P, I64, P, C.c_uint32, I32, P, P]),
    "svr_gather_fc0_bf16_prepare": (C.c_int, [C.POINTER(GatherDesc), P, I64, I32, P, P]),
    "svr_gather_fc0_bf16_run": (C.c_int, [C.POINTER(GatherDesc), P, P, P, I64, I32, I32, P, P]),
    "svr_gather_trilinear_bwd": (C.c_int, [C.POINTER(GatherDesc), P, P, P, P]),
    "svr_gather_corner_indices": (C.c_int, [C.POINTER(GatherDesc), I32, P, P, P]),
    "svr_cast_f32_to_bf16": (C.c_int, [P, P, I64, P]),
    "svr_gather_trilinear_fwd_bf16": (C.c_int, [C.POINTER(GatherDesc), P, P, P]),
    "svr_linear_fwd_bf16": (C.c_int, [P, I64, P, I64, P, P, I64, I64, I64, I64, C.c_int, P]),
    "svr_fc_out_fwd_bf16": (C.c_int, [P, I64, P, P, P, P, I64, I64, P]),
    "svr_linear_fwd": (C.c_int, [P, I64, P, I64, P, P, I64, I64, I64, I64, C.c_int, P, I64, P]),
    "svr_linear_bwd_data": (C.c_int, [P, I64, P, I64, P, I64, I64, I64, I64, C.c_int, P, I64, P]),
    "svr_linear_bwd_weight_workspace": (I64, [I64, I64, I64]),
    "svr_linear_bwd_weight": (C.c_int, [P, I64, P, I64, P, I64, P, I64, I64, I64, P, P]),
    "svr_linear_fwd_bf16x6_workspace": (I64, [I64, I64]),
    "svr_linear_fwd_bf16x6": (C.c_int, [P, I64, P, I64, P, P, I64, I64, I64, I64, C.c_int, P, P]),
    "svr_linear_fwd_f16x3_workspace": (I64, [I64, I64]),
    "svr_linear_fwd_f16x3": (C.c_int, [P, I64, P, I64, P, P, I64, I64, I64, I64, C.c_int, P, P]),
    "svr_linear_bwd_data_bf16x3_workspace": (I64, [I64, I64]),
    "svr_linear_bwd_data_bf16x3": (C.c_int, [P, I64, P, I64, P, I64, I64, I64, I64, C.c_int, P, I64, P, P]),
    "svr_linear_bwd_weight_bf16x3_workspace": (I64, [I64, I64, I64]),
    "svr_linear_bwd_weight_bf16x3": (C.c_int, [P, I64, P, I64, P, I64, P, I64, I64, I64, P, P]),
    "svr_amax_f32": (C.c_int, [P, I64, I64, I64, P, P]),
    "svr_linear_bwd_data_f16x3_workspace": (I64, [I64, I64]),
    "svr_linear_bwd_data_f16x3": (C.c_int, [P, I64, P, I64, P, I64, I64, I64, I64, C.c_int, P, I64, P, P, P, P]),
    "svr_linear_bwd_weight_f16x3_workspace": (I64, [I64, I64, I64]),
    "svr_linear_bwd_weight_f16x3": (C.c_int, [P, I64, P, I64, P, I64, P, I64, I64, I64, P, P, P]),
    "svr_linear_variant": (C.c_int, [I32, I64, I64, I64, I64, I64, I64, I64, I32, I32, I32, I32, I32, I32, P, P, P, P, P, P]),
    "svr_fc_out_fwd": (C.c_int, [P, I64, P, P, P, P, I64, I64, P]),
    "svr_mlp_tail_fwd_workspace": (I64, [I64]),
    "svr_mlp_tail_fwd": (C.c_int, [P, I64, P, P, P, P, P, P, P, I64, P, I64, P, P, I64, I64, P, P]),
    "svr_fc_out_bwd_workspace": (I64, [I64, I64]),
    "svr_fc_out_bwd": (C.c_int, [P, I64, P, P, P, P, I64, P, P, I64, I64, P, P, P]),
    "svr_bce_logits_sum_mean": (C.c_int, [P, P, P, P, I64, I64, F32, P, P]),
    "svr_bce_ordered_workspace": (I64, [I64]),
    "svr_bce_logits_sum_mean_ordered": (C.c_int, [P, P, P, P, I64, I64, F32, P, P]),
    "svr_conv3d_pack_weight": (C.c_int, [P, P, P, I32, I32, P]),
    "svr_conv3d_unpack_wgrad": (C.c_int, [P, P, I32, I32, P]),
    "svr_conv3d_k3": (C.c_int, [P, P, P, P, I32, I32, I32, I32, I32, I32, C.c_int, P, P]),
    "svr_conv3d_fwd_bf16x6_workspace": (I64, [I32, I32]),
    "svr_conv3d_k3_fwd_bf16x6": (C.c_int, [P, P, P, P, I32, I32, I32, I32, I32, I32, C.c_int, P, P]),
    "svr_conv3d_fwd_f16x3_workspace": (I64, [I32, I32]),
    "svr_conv3d_k3_fwd_f16x3": (C.c_int, [P, P, P, P, I32, I32, I32, I32, I32, I32, C.c_int, P, P]),
    "svr_conv3d_fwd_f16x3_stats_blocks": (I32, [I32, I32, I32, I32, I32, I32]),
    "svr_conv3d_k3_fwd_f16x3_stats": (C.c_int, [P, P, P, P, P, I32, I32, I32, I32, I32, I32, C.c_int, P, P]),
    "svr_conv3d_bwd_data_bf16x3_workspace": (I64, [I32, I32]),
    "svr_conv3d_k3_bwd_data_bf16x3": (C.c_int, [P, P, P, I32, I32, I32, I32, I32, I32, C.c_int, P, P, P]),
    "svr_conv3d_c1_fwd_stats_workspace": (I64, [I32, I32, I32, I32, I32]),
    "svr_conv3d_c1_fwd_stats": (C.c_int, [P, P, P, P, P, I32, I32, I32, I32, I32, C.c_int, P, P]),
    "svr_conv3d_k3_bwd_weight_workspace": (I64, [I32, I32, I32, I32, I32, I32]),
    "svr_conv3d_k3_bwd_weight": (C.c_int, [P, P, P, P, I32, I32, I32, I32, I32, I32, P, P]),
    "svr_conv3d_k3_bwd_weight_bf16x3_workspace": (I64, [I32, I32, I32, I32, I32, I32]),
    "svr_conv3d_k3_bwd_weight_bf16x3": (C.c_int, [P, P, P, P, I32, I32, I32, I32, I32, I32, P, P]),
    "svr_conv3d_k3_bwd_weight_bf16x3_param": (C.c_int, [P, P, P, P, I32, I32, I32, I32, I32, I32, P, P]),
    "svr_conv3d_bwd_data_f16x3_workspace": (I64, [I32, I32]),
    "svr_conv3d_k3_bwd_data_f16x3": (C.c_int, [P, P, P, I32, I32, I32, I32, I32, I32, C.c_int, P, P, P, P, P]),
    "svr_conv3d_k3_bwd_weight_f16x3": (C.c_int, [P, P, P, P, I32, I32, I32, I32, I32, I32, I32, P, P, P]),
    "svr_conv3d_k3_variant": (C.c_int, [I32, I32, I32, I32, I32, I32, I32, P, P, P, P, P]),
    "svr_conv3d_k3_bwd_weight_variant": (C.c_int, [I32, I32, I32, I32, I32, I32, I32, P, P, P]),
    "svr_bn_stats_workspace": (I64, [I64, I32]),
    "svr_bn_stats": (C.c_int, [P, P, I64, I32, P, P]),
    "svr_bn_stats_finalize": (C.c_int, [P, P, P, P, P, P, P, P, P, I64, I32, F32, F32, P, P]),
    "svr_bn_finalize_parts": (C.c_int, [P, I32, P, P, P, P, P, P, P, P, I64, I32, F32, F32, P]),
    "svr_bn_finalize": (C.c_int, [P, P, P, P, P, P, P, I64, I32, F32, F32, C.c_int, P]),
    "svr_bn_apply_pool": (C.c_int, [P, P, P, P, P, P, P, P, I32, I32, I32, I32, I32, P]),
    "svr_bn_bwd_reduce": (C.c_int, [P, P, P, P, P, P, P, P, I32, I32, I32, I32, I32, P, P]),
    "svr_bn_bwd_apply": (C.c_int, [P, P, P, P, P, P, P, P, P, P, P, P, I32, I32, I32, I32, I32, C.c_int, P, P]),
    "svr_stage1_supported": (I32, [I32, I32, I32, I32, I32]),
    "svr_stage1_workspace": (I64, [I32, I32, I32, I32]),
    "svr_stage1_fwd": (C.c_int, [P, P, P, P, P, P, P, P, P, P, P, P, P, I32, I32, I32, I32, I32, F32, F32, C.c_int, C.c_int, P, P]),
    "svr_stage1_bwd": (C.c_int, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, I32, I32, I32, I32, I32, C.c_int, C.c_int, P, P]),
    "svr_conv2d_im2col": (C.c_int, [C.POINTER(Conv2dDesc), P, P]),
    "svr_conv2d_col2im": (C.c_int, [C.POINTER(Conv2dDesc), P, P, P, P, P]),
    "svr_conv2d_small_supported": (C.c_int, [I32, I32, I32]),
    "svr_conv2d_small_fwd": (C.c_int, [C.POINTER(Conv2dDesc), P, P, P, I32, P]),
    "svr_conv2d_small_bwd_data": (C.c_int, [C.POINTER(Conv2dDesc), P, P, I32, P, P]),
    "svr_conv2d_small_bwd_weight_workspace": (I64, [C.POINTER(Conv2dDesc), I32]),
    "svr_conv2d_small_bwd_weight": (C.c_int, [C.POINTER(Conv2dDesc), P, I32, P, P, P, P]),
    "svr_conv2d_planes_bytes": (I64, [I32, I32, I32]),
    "svr_conv2d_prepare": (C.c_int, [P, I32, I32, I32, I32, I32, P, P, P]),
    "svr_conv2d_prepare_many": (C.c_int, [I32, P, P, P, P, P, P, P, P, P]),
    "svr_conv2d_workspace_bytes": (I64, [C.POINTER(Conv2dDesc), I32]),
    "svr_conv2d_virtual": (C.c_int, [C.POINTER(Conv2dDesc), P, P]),
    "svr_conv2d_fwd": (C.c_int, [C.POINTER(Conv2dDesc), P, P, P, P, I32, P, P, P, P]),
    "svr_conv2d_bwd_data": (C.c_int, [C.POINTER(Conv2dDesc), P, P, P, P, I32, P, P, P]),
    "svr_conv2d_finish_bwd": (C.c_int, [C.POINTER(Conv2dDesc), P, P, P, P]),
    "svr_conv2d_bwd_weight_workspace": (I64, [C.POINTER(Conv2dDesc), I32]),
    "svr_conv2d_bwd_weight": (C.c_int, [C.POINTER(Conv2dDesc), P, P, I32, P, P, P, P]),
    "svr_conv2d_variant": (C.c_int, [I32] * 13 + [C.POINTER(Conv2dPlan)]),
    "svr_mesh_hash_entries": (I64, [P, I64, P, I64, I32, P]),
    "svr_mesh_hash_build": (C.c_int, [P, I64, P, I64, I32, P, P, P, I64]),
    "svr_mesh_contains": (C.c_int, [P, I32, I64, P, P, P, I32, P, P, P, P]),
    "svr_mesh_face_table": (C.c_int, [P, I64, P, I64, P, P]),
    "svr_mesh_sample": (C.c_int, [P, P, I64, P, I64, P, P, P]),
    "svr_nn_search_workspace": (I64, [I64]),
    "svr_nn_search": (C.c_int, [P, I64, P, I64, P, P, P, I64, P]),
    "svr_nn_normals_dot": (C.c_int, [P, P, I32, P, I64, I64, P, P]),
    "svr_eval_sums": (C.c_int, [P, P, I64, P, P, I64, P]),
    "svr_iou_counts": (C.c_int, [P, P, I64, P, P]),
    "svr_mesh_df_bricks": (I64, [I32, I32, I32, I32]),
    "svr_mesh_df_workspace_bytes": (I64, [I32, I32, I32, I32]),
    "svr_mesh_df_valid_faces": (C.c_int, [P, I64, P, P, P]),
    "svr_mesh_df_count": (C.c_int, [P, I64, I32, I32, I32, I32, C.c_double, C.c_double, P, I64, P, P]),
    "svr_mesh_df_emit": (C.c_int, [P, I64, I32, I32, I32, I32, P, P, I64, I64, P, I64, P]),
    "svr_mesh_df_eval": (C.c_int, [P, I64, I32, I32, I32, I32, C.c_double, P, P, I64, I64, P, P, P]),
    "svr_raycast_tiles": (I64, [I32, I32, I32]),
    "svr_raycast_workspace_bytes": (I64, [I32, I32, I32]),
    "svr_raycast_face_bounds": (C.c_int, [P, I64, C.POINTER(F32), P, P]),
    "svr_raycast_count": (C.c_int, [P, I64, I32, I32, I32, P, I64, P, P]),
    "svr_raycast_emit": (C.c_int, [P, I64, I32, I32, I32, P, I64, I64, P, I64, P]),
    "svr_raycast_eval": (C.c_int, [P, I64, C.POINTER(F32), I32, I32, I32, C.c_double, C.c_double, F32, P, P, I64, I64, P, P, P,
                                   P, P, P]),
    "svr_vertex_color_workspace_bytes": (I64, [I64]),
    "svr_vertex_color_sample": (C.c_int, [P, I64, C.POINTER(F32), P, I32, I32, C.c_double, P, I32, I32, C.POINTER(C.c_double),
                                          C.POINTER(C.c_uint8), P, P, P]),
    "svr_vertex_color_spread": (C.c_int, [P, I64, I64, P, P, P, I64, I64, I32, C.POINTER(I64), P]),
    "svr_mesh_components_workspace_bytes": (I64, [I64, I64]),
    "svr_mesh_components_label": (C.c_int, [P, I64, I64, P, I64, P, P, P, P]),
    "svr_mesh_components_stats": (C.c_int, [P, I64, P, P, I64, P, I64, P, I64, P, P, P, P, P, P, I32, P]),
    "svr_mesh_filter_count": (C.c_int, [P, I64, I64, P, P, I64, P, I64, P, P]),
    "svr_mesh_filter_emit": (C.c_int, [P, I64, P, I64, P, I64, P, P, P, P]),
    "svr_mesh_simplify_workspace_bytes": (I64, [I64, I64]),
    "svr_mesh_simplify_count": (C.c_int, [P, I64, P, I64, F32, P, I64, I32, P, P]),
    "svr_mesh_simplify_emit": (C.c_int, [P, I64, P, I64, P, I64, P, P, P, P, P]),
    "svr_mesh_smooth_workspace_bytes": (I64, [I64, I64]),
    "svr_mesh_smooth": (C.c_int, [P, I64, P, I64, I32, F32, F32, I32, P, I64, P, P, P, P]),
    "svr_mesh_vertex_normals_workspace_bytes": (I64, [I64, I64]),
    "svr_mesh_vertex_normals": (C.c_int, [P, I64, P, I64, P, I64, P, P, P, P]),
    "svr_mesh_shade": (C.c_int, [P, P, I64, I64, P, C.POINTER(F32), I32, I32, P, P, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), F32, P, P]),
    "svr_box_downsample_rgb8": (C.c_int, [P, I32, I32, I32, P, P]),
    "svr_mc_workspace_bytes": (I64, [I32, I32, I32]),
    "svr_mc_count": (C.c_int, [P, I32, I32, I32, C.c_double, P, I64, P, P]),
    "svr_mc_emit": (C.c_int, [P, I32, I32, I32, C.c_double, P, P, P, P]),
    "svr_mc_case_table": (C.c_int, [P]),
    "svr_sl_workspace_bytes": (I64, [I32, I32, I32, I32]),
    "svr_sl_coarse_points": (C.c_int, [P, P, P, I32, I32, I32, I32, P, P]),
    "svr_sl_fill_seed": (C.c_int, [P, I32, I32, I32, I32, C.c_double, P, P, P, I64, P]),
    "svr_sl_select": (C.c_int, [I32, I32, I32, I32, I32, P, P, P, P]),
    "svr_sl_block_points": (C.c_int, [P, P, P, I32, I32, I32, I32, P, I64, P, P]),
    "svr_sl_scatter": (C.c_int, [P, I32, I32, I32, I32, P, I64, I32, P, P, P]),
    "svr_sl_leak_check": (C.c_int, [P, I32, I32, I32, I32, C.c_double, P, P, I64, P, P]),
    "svr_df_to_grid": (C.c_int, [P, P, I32, I32, I32, P]),
    "svr_cast_to_f32": (C.c_int, [P, I32, P, I64, P]),
    "svr_subsample_rows": (C.c_int, [P, I32, I64, I32, P, I64, P, P, P]),
    "svr_subsample_rows_batched": (C.c_int, [P, P, I32, I64, P, P, P, P]),
    "svr_distance_to_depth": (C.c_int, [P, P, I32, I32, I32, F32, P]),
    "svr_depth_grid_mark": (C.c_int, [P, I32, F32, I32, I32, C.POINTER(F32), P, I32, I32, I32, P, P, P]),
    "svr_unproject_fwd": (C.c_int, [P, P, I32, I32, I32, C.POINTER(F32), C.c_int, P]),
    "svr_unproject_bwd": (C.c_int, [P, P, P, I32, I32, I32, C.POINTER(F32), C.c_int, P]),
    "svr_voxelize_splat_fwd": (C.c_int, [P, P, P, P, I32, I32, I32, I32, I32, P]),
    "svr_voxelize_splat_bwd": (C.c_int, [P, P, P, I32, I32, I32, I32, I32, P]),
    "svr_scale_clamp01_fwd": (C.c_int, [P, P, I64, F32, P]),
    "svr_scale_clamp01_bwd": (C.c_int, [P, P, P, I64, F32, P]),
    "svr_blur_axis_fwd": (C.c_int, [P, P, P, I32, I32, I32, I32, I32, I32, P]),
    "svr_blur_axis_bwd": (C.c_int, [P, P, P, P, P, I32, I32, I32, I32, I32, I32, P]),
    "svr_voxelize_splat_ordered_workspace": (I64, [I32, I32, I32, I32, I32]),
    "svr_voxelize_splat_fwd_ordered": (C.c_int, [P, P, P, P, P, I32, I32, I32, I32, I32, P, P]),
    "svr_blur_axis_bwd_ordered_workspace": (I64, [I32, I32, I32, I32, I32]),
    "svr_blur_axis_bwd_ordered": (C.c_int, [P, P, P, P, P, I32, I32, I32, I32, I32, I32, P, P]),
    "svr_voxel_mesh_workspace_bytes": (I64, [I32, I32, I32]),
    "svr_voxel_mesh_count": (C.c_int, [P, I32, I32, I32, C.c_double, P, I64, P, P]),
    "svr_voxel_mesh_emit": (C.c_int, [P, I32, I32, I32, C.c_double, P, P, P, P]),
    "svr_depth_minmax": (C.c_int, [P, I64, P, P]),
    "svr_depth_planes": (C.c_int, [P, I32, I32, I32, P, P, P, P]),
    "svr_depth_head_workspace": (I64, [I32, I32, I32]),
    "svr_depth_head_fwd": (C.c_int, [P, P, P, P, P, I32, I32, I32, I32, I32, I32, C.c_double, C.c_double, P, P]),
    "svr_depth_head_bwd": (C.c_int, [P, P, I32, I32, I32, I32, I32, I32, P]),
    "svr_rgb_resize_taps": (I32, [I32, I32]),
    "svr_rgb_resize_table": (C.c_int, [I32, I32, I32, P]),
    "svr_rgb_preprocess": (C.c_int, [P, I32, I32, I32, I32, I32, I32, P, I32, P, I32, P, P, P, P, P]),
    "svr_grid_to_camera": (C.c_int, [P, P, I64, C.POINTER(F32), P]),
    # file formats (csrc/io_*.cpp): host pointers only, no stream, no GPU needed
    "svr_write_obj": (C.c_int, [C.c_char_p, P, I64, P, I64]),
    "svr_write_ply": (C.c_int, [C.c_char_p, P, P, I64, P, I64]),
    "svr_write_png_gray8": (C.c_int, [C.c_char_p, P, I32, I32]),
    "svr_write_png_rgb8": (C.c_int, [C.c_char_p, P, I32, I32]),
    "svr_write_obj_normals": (C.c_int, [C.c_char_p, P, P, I64, P, I64]),
    "svr_write_obj_points": (C.c_int, [C.c_char_p, P, I64]),
    "svr_df_dims": (C.c_int, [C.c_char_p, P]),
    "svr_df_read": (C.c_int, [C.c_char_p, P, I64]),
    "svr_df_write": (C.c_int, [C.c_char_p, P, I64, I64, I64]),
    "svr_npz_member_info": (C.c_int, [C.c_char_p, C.c_char_p, P, P, P, P]),
    "svr_npz_member_read": (C.c_int, [C.c_char_p, C.c_char_p, P, I64]),
    "svr_exr_info": (C.c_int, [C.c_char_p, P, P, P, P, P, I64, P, I32, P, P]),
    "svr_exr_read_channel": (C.c_int, [C.c_char_p, C.c_char_p, P, I64]),
    "svr_exr_write": (C.c_int, [C.c_char_p, P, I32, I32, C.c_char_p, I32]),
}

_lib = None


def lib():
    """Load (once) and return the bound library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the HIP path.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)          # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        # layout pin: the ctypes mirrors above against the structs the library was compiled with
        if l.svr_sizeof_level() != C.sizeof(Level) or l.svr_sizeof_gather_desc() != C.sizeof(GatherDesc):
            raise RuntimeError(f"svr_level / svr_gather_desc layout mismatch: library {l.svr_sizeof_level()} / "
                               f"{l.svr_sizeof_gather_desc()} bytes, binding {C.sizeof(Level)} / {C.sizeof(GatherDesc)}")
        _lib = l
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().svr_last_error()
        raise RuntimeError(f"libsvr_hip {what} failed (rc={rc}): {msg.decode(errors='replace') if msg else ''}")


# ---- what every binding module passes to the library ------------------------------------------------------------------
def stream():
    """The current HIP stream as the library's `void *stream`."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a contiguous GPU tensor; None -> NULL."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise RuntimeError("svr_amd ops need GPU tensors (the HIP path has no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError("svr_amd ops need contiguous tensors")
    return C.c_void_p(t.data_ptr())


def to_device(a, what, dtype=None, device=None):
    """The input convention of the data-processing / evaluation entry points: a numpy array (or anything np.asarray
    takes) is uploaded and the caller hands numpy back, a device tensor stays on the device, a CPU tensor is refused.
    -> (contiguous device tensor [cast to `dtype`], came_from_numpy)."""
    as_numpy = not torch.is_tensor(a)
    if as_numpy:        # (a float target type is cast on the host: numpy takes every source type, and rounds like the device)
        a = np.ascontiguousarray(np.asarray(a), dtype={torch.float32: np.float32, torch.float64: np.float64}.get(dtype))
        a = torch.from_numpy(a).to(device if device is not None else "cuda")
    elif not a.is_cuda:
        raise RuntimeError(f"{what} HIP path needs GPU tensors (no CPU fallback)")
    if dtype is not None and a.dtype != dtype:
        a = a.to(dtype)
    return a.contiguous(), as_numpy
