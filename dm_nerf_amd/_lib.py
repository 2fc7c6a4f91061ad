"""ctypes binding of libdmnerf_hip.so (the C ABI declared in include/dmnerf_hip.h).

PyTorch is plumbing only: it owns device memory and streams; every pointer handed to the
library is ``tensor.data_ptr()`` and every launch goes to ``torch.cuda.current_stream()``.
"""
import ctypes
import os

import numpy as np
import torch  # must be imported first: the library binds to the HIP runtime torch already loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdmnerf_hip.so")

c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_vp = ctypes.c_void_p
c_float = ctypes.c_float
c_double = ctypes.c_double


class RenderArgs(ctypes.Structure):
    """``dmnerf_render_args`` (include/dmnerf_hip.h)."""
    _fields_ = [
        ("d_blob_coarse", c_vp), ("d_blob_fine", c_vp), ("ins_num", c_int),
        ("d_rays_o", c_vp), ("d_rays_d", c_vp), ("d_z_in", c_vp), ("d_t_rand", c_vp), ("d_u", c_vp),
        ("u_row_stride", c_i64), ("N", c_i64), ("S", c_int), ("n_imp", c_int),
        ("d_z_coarse", c_vp), ("d_raw_coarse", c_vp), ("d_rgb_coarse", c_vp), ("d_depth_coarse", c_vp),
        ("d_ins_coarse", c_vp), ("d_z_fine", c_vp), ("d_raw_fine", c_vp), ("d_rgb_fine", c_vp),
        ("d_depth_fine", c_vp), ("d_ins_fine", c_vp), ("d_weights_ws", c_vp),
        ("ev_fine_mlp_begin", c_vp), ("ev_fine_mlp_end", c_vp), ("fused_heads", c_int),
    ]


class RenderFineArgs(ctypes.Structure):
    """``dmnerf_render_fine_args`` (include/dmnerf_hip.h)."""
    _fields_ = [
        ("d_blob_coarse", c_vp), ("d_blob_fine", c_vp), ("ins_num", c_int),
        ("d_rays_o", c_vp), ("d_rays_d", c_vp), ("d_z_in", c_vp), ("d_t_rand", c_vp), ("d_u", c_vp),
        ("u_row_stride", c_i64), ("N", c_i64), ("S", c_int), ("n_imp", c_int),
        ("d_z_coarse", c_vp), ("d_sigma_ws", c_vp), ("d_weights_ws", c_vp),
        ("d_z_fine", c_vp), ("d_raw_fine", c_vp), ("d_rgb_fine", c_vp), ("d_depth_fine", c_vp), ("d_ins_fine", c_vp),
        ("ev_fine_mlp_begin", c_vp), ("ev_fine_mlp_end", c_vp), ("fused_heads", c_int),
    ]


class SkipGridArgs(ctypes.Structure):
    """``dmnerf_skip_grid`` (include/dmnerf_hip.h)."""
    _fields_ = [("lo", c_float * 3), ("inv_cell", c_float * 3), ("dims", c_int * 3), ("outside", c_int), ("d_bits", c_vp)]


class RenderFineSkipArgs(ctypes.Structure):
    """``dmnerf_render_fine_skip_args`` (include/dmnerf_hip.h)."""
    _fields_ = [("fine", RenderFineArgs), ("grid", SkipGridArgs), ("d_sel", c_vp), ("d_n_eval", c_vp), ("d_flag", c_vp),
                ("d_select_ws", c_vp), ("levels", c_int)]


class RepackModel(ctypes.Structure):
    """``dmnerf_repack_model`` (include/dmnerf_hip.h)."""
    _fields_ = [("d_params_flat", c_vp), ("ins_num", c_int), ("d_flat_copy", c_vp), ("d_idx", c_vp), ("d_blob", c_vp),
                ("d_idx_t", c_vp), ("d_blob_t", c_vp), ("d_f_pos", c_vp)]


class ChainLayer(ctypes.Structure):
    """``dmnerf_chain_layer`` (include/dmnerf_hip.h)."""
    _fields_ = [("d_B", c_vp), ("d_bias", c_vp), ("ldb", c_int), ("from_act", c_int), ("from_x", c_int), ("relu", c_int)]


class VolumeEditEntry(ctypes.Structure):
    """``dmnerf_volume_edit_entry`` (include/dmnerf_hip.h)."""
    _fields_ = [("kind", c_int), ("label", c_int), ("m", c_float * 12)]


# name -> (restype, argtypes); exactly the symbols include/dmnerf_hip.h declares
SIGNATURES = {
    "dmnerf_adam_step": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_double, c_vp, c_double, c_double, c_double, c_vp, c_vp]),
    "dmnerf_repack_train": (c_int, [ctypes.POINTER(RepackModel), c_int, c_vp]),
    "dmnerf_abi_version": (c_int, []),
    "dmnerf_last_error": (ctypes.c_char_p, []),
    "dmnerf_device_count": (c_int, []),
    "dmnerf_param_count": (c_i64, [c_int]),
    "dmnerf_blob_floats": (c_i64, [c_int]),
    "dmnerf_build_pack_index": (c_int, [c_int, c_vp, c_i64]),
    "dmnerf_pack_weights": (c_int, [c_vp, c_vp, c_vp, c_i64, c_vp]),
    "dmnerf_raygen": (c_int, [c_int, c_int, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_raygen_select": (c_int, [c_int, c_int, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "dmnerf_z_val_sample": (c_int, [c_vp, c_float, c_float, c_i64, c_int, c_vp, c_vp]),
    "dmnerf_stratify": (c_int, [c_vp, c_vp, c_i64, c_int, c_vp, c_vp]),
    "dmnerf_sample_pdf": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_sample_from_cdf": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_importance_resample": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_embed": (c_int, [c_vp, c_i64, c_int, c_vp, c_vp]),
    "dmnerf_mlp_fwd_embedded": (c_int, [c_vp, c_int, c_vp, c_i64, c_vp, c_vp]),
    "dmnerf_mlp_fwd_rays": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp]),
    "dmnerf_composite_fwd": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_render_rays_fwd": (c_int, [ctypes.POINTER(RenderArgs), c_vp]),
    "dmnerf_mlp_fwd_rays_density": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp]),
    "dmnerf_weights_from_sigma": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp]),
    "dmnerf_render_rays_fwd_fine": (c_int, [ctypes.POINTER(RenderFineArgs), c_vp]),
    "dmnerf_mlp_fwd_points_density": (c_int, [c_vp, c_int, c_vp, c_i64, c_vp, c_float, c_vp]),
    "dmnerf_occupancy_slab": (c_int, [c_vp, c_int, c_vp, c_int, ctypes.POINTER(c_float), ctypes.POINTER(c_float), c_i64, c_i64, c_vp, c_float, c_vp]),
    "dmnerf_composite_bwd": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp, c_vp]),
    "dmnerf_train_save_floats": (c_i64, [c_i64]),
    "dmnerf_mlp_fwd_embedded_train": (c_int, [c_vp, c_int, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "dmnerf_mlp_fwd_rays_train_split": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_mlp_fwd_rays_train_fused": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_mlp_fwd_rays_train": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_blob_t_floats": (c_i64, [c_int]),
    "dmnerf_build_pack_index_t": (c_int, [c_int, c_vp, c_i64]),
    "dmnerf_mlp_bwd_data": (c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "dmnerf_manipulator_render": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_z_val_lerp": (c_int, [c_vp, c_float, c_float, c_i64, c_int, c_vp, c_vp]),
    "dmnerf_sort_rows": (c_int, [c_vp, c_i64, c_int, c_vp, c_vp]),
    "dmnerf_ins_label_conf": (c_int, [c_vp, c_i64, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_exchanger": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_i64, c_int, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_edit_exchange": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_i64, c_int, c_int, c_vp, c_vp]),
    "dmnerf_edit_rays": (c_int, [c_int, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_vp, c_vp]),
    "dmnerf_edit_products": (c_int, [c_vp, c_i64, c_vp, c_i64, c_int, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_penalizer_fwd": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_float, c_float, c_float, c_vp, c_vp]),
    "dmnerf_penalizer_bwd": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_float, c_float, c_float, c_vp, c_vp, c_vp]),
    "dmnerf_penalizer_sums": (c_int, [c_vp, c_i64, c_vp, c_vp]),
    "dmnerf_penalizer_finish": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_f16x2_range_flags": (c_int, [c_vp, c_i64, c_int, c_vp, c_vp]),
    "dmnerf_penalizer_sums2": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp]),
    "dmnerf_loss_tail_fwd": (c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_loss_tail_bwd": (c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_composite_pen_fwd": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_float, c_float, c_float, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_composite_pen_bwd": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_float, c_float, c_float, c_vp, c_vp]),
    "dmnerf_wgrad_plan_sizes": (c_int, [c_int, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_wgrad_plan": (c_int, [c_int, c_i64, c_int, c_vp, c_i64, c_vp, c_i64]),
    "dmnerf_mlp_bwd_weights": (c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_wgrad_plan_sizes_split": (c_int, [c_int, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_wgrad_plan_split": (c_int, [c_int, c_i64, c_int, c_vp, c_i64, c_vp, c_i64]),
    "dmnerf_wgrad_plan_sizes_f16": (c_int, [c_int, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_wgrad_plan_f16": (c_int, [c_int, c_i64, c_int, c_vp, c_i64, c_vp, c_i64]),
    "dmnerf_mlp_bwd_weights_split": (c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_head_product": (c_int, [c_vp, c_int, c_vp, c_vp]),
    "dmnerf_fuse_heads": (c_int, [c_vp, c_int, c_vp, c_vp]),
    "dmnerf_gemm": (c_int, [c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_int, c_i64, c_vp, c_int, c_vp, c_i64, c_int, c_vp, c_int, c_vp]),
    "dmnerf_colsum": (c_int, [c_vp, c_i64, c_i64, c_int, c_vp, c_vp, c_int, c_vp]),
    "dmnerf_ray_points": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_copy_cols": (c_int, [c_vp, c_i64, c_vp, c_i64, c_i64, c_int, c_vp]),
    "dmnerf_gemm_nt_blocks": (c_int, [c_int]),
    "dmnerf_pack_nt": (c_int, [c_vp, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_int, c_int, c_vp, c_vp]),
    "dmnerf_gemm_nt": (c_int, [c_vp, c_i64, c_i64, c_int, c_vp, c_i64, c_i64, c_int, c_vp, c_i64, c_int, c_vp, c_vp, c_i64, c_int, c_int,
                               c_i64, c_int, c_vp, c_i64, c_int, c_vp]),
    "dmnerf_gemm_tn_ws_floats": (c_i64, [c_int, c_int, c_i64]),
    "dmnerf_gemm_tn": (c_int, [c_vp, c_i64, c_i64, c_int, c_vp, c_i64, c_i64, c_int, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
    "dmnerf_mlp_chain_supported": (c_int, [c_int, c_int]),
    "dmnerf_mlp_chain": (c_int, [c_vp, c_i64, c_i64, c_int, ctypes.POINTER(ChainLayer), c_int, c_int, c_vp, c_i64, c_i64, c_vp]),
    "dmnerf_copy_cols_pad": (c_int, [c_vp, c_i64, c_vp, c_i64, c_i64, c_int, c_int, c_vp]),
    "dmnerf_ray_embed": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_int, c_vp, c_int, c_vp, c_int, c_vp]),
    "dmnerf_wgrad_set_trace": (c_int, [c_vp]),
    "dmnerf_blob_split_words": (c_i64, [c_int]),
    "dmnerf_build_pack_index_split": (c_int, [c_int, c_vp, c_i64]),
    "dmnerf_pack_split": (c_int, [c_vp, c_vp, c_vp, c_i64, c_vp]),
    "dmnerf_blob_t_split_words": (c_i64, [c_int]),
    "dmnerf_build_pack_index_t_split": (c_int, [c_int, c_vp, c_i64]),
    "dmnerf_mlp_bwd_data_split": (c_int, [c_vp, c_int, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "dmnerf_mlp_fwd_rays_split": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp]),
    "dmnerf_blob_f16_words": (c_i64, [c_int]),
    "dmnerf_build_pack_index_f16": (c_int, [c_int, c_vp, c_i64, c_vp, c_i64]),
    "dmnerf_pack_f16": (c_int, [c_vp, c_vp, c_vp, c_i64, c_vp]),
    "dmnerf_mlp_fwd_rays_f16": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp]),
    "dmnerf_blob_t_f16_words": (c_i64, [c_int]),
    "dmnerf_build_pack_index_t_f16": (c_int, [c_int, c_vp, c_i64]),
    "dmnerf_grad_scale": (c_int, [c_vp, c_i64, c_vp, c_vp]),
    "dmnerf_mlp_bwd_data_f16": (c_int, [c_vp, c_int, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_mlp_bwd_weights_f16": (c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_mlp_fwd_rays_train_f16": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_blob_fused_floats": (c_i64, [c_int]),
    "dmnerf_build_pack_index_fused": (c_int, [c_int, c_vp, c_i64]),
    "dmnerf_mlp_fwd_rays_fused": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp]),
    "dmnerf_ins_criterion_work_bytes": (c_i64, [c_i64, c_int]),
    "dmnerf_ins_criterion_flags_offset": (c_i64, [c_i64, c_int]),
    "dmnerf_ins_criterion_fwd": (c_int, [c_vp, c_vp, c_i64, c_int, c_vp, c_i64, c_vp, c_vp]),
    "dmnerf_ins_criterion_bwd": (c_int, [c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_ins_criterion_fwd2": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "dmnerf_ins_criterion_bwd2": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_ins_eval_work_bytes": (c_i64, [c_i64, c_int]),
    "dmnerf_ins_eval_flags_offset": (c_i64, [c_i64, c_int]),
    "dmnerf_ins_eval_median_offset": (c_i64, [c_i64, c_int]),
    "dmnerf_ins_eval_prep": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_int, c_i64, c_int, c_vp, c_i64, c_vp]),
    "dmnerf_ins_eval": (c_int, [c_i64, c_int, c_int, c_int, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "dmnerf_img_metrics_work_bytes": (c_i64, [c_int, c_int, c_int, c_int]),
    "dmnerf_img_metrics": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_conv3x3_pack": (c_int, [c_vp, c_int, c_int, c_vp, c_int, c_vp]),
    "dmnerf_conv3x3": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "dmnerf_maxpool2": (c_int, [c_vp, c_i64, c_vp, c_i64, c_int, c_int, c_int, c_int, c_vp]),
    "dmnerf_lpips_prologue": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_i64, c_vp]),
    "dmnerf_lpips_tail": (c_int, [c_vp, c_i64, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_i64, c_vp, c_vp]),
    "dmnerf_lpips_work_bytes": (c_i64, [c_int, c_int, c_int]),
    "dmnerf_surface_count": (c_int, [c_vp, c_int, c_int, c_int, c_float, c_vp, c_vp, c_vp]),
    "dmnerf_surface_emit": (c_int, [c_vp, c_int, c_int, c_int, c_float, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp]),
    "dmnerf_surface_normals": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_surface_clusters": (c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_surface_clean_mark": (c_int, [c_vp, c_i64, c_i64, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_surface_clean_compact": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_object_surface_count": (ctypes.c_int32, [c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_uint32), c_float, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_object_surface_emit": (ctypes.c_int32, [c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_uint32), c_float, c_int, c_vp, c_vp, c_vp,
                                           c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_object_surface_measures": (ctypes.c_int32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_int, ctypes.POINTER(c_double), c_vp, c_vp, c_vp]),
    "dmnerf_skip_grid_build": (c_int, [c_vp, c_int, c_int, c_int, c_float, c_int, c_vp, c_vp]),
    "dmnerf_skip_select_work_ints": (c_i64, [c_i64]),
    "dmnerf_skip_select": (c_int, [ctypes.POINTER(SkipGridArgs), c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_skip_select_fill": (c_int, [ctypes.POINTER(SkipGridArgs), c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                        c_int, c_vp, c_vp]),
    "dmnerf_mlp_fwd_rays_sel": (c_int, [c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_mlp_fwd_rays_density_sel": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_blob_f16_density_words": (c_i64, [c_int]),
    "dmnerf_blob_f16_density_from_f16": (c_int, [c_vp, c_int, c_vp, c_vp]),
    "dmnerf_mlp_fwd_rays_density_f16": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp]),
    "dmnerf_mlp_fwd_rays_f16_sel": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_mlp_fwd_rays_density_f16_sel": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_render_rays_fwd_fine_skip": (c_int, [ctypes.POINTER(RenderFineSkipArgs), c_vp]),
    "dmnerf_skip_grid_mark": (c_int, [ctypes.POINTER(SkipGridArgs), c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_float, c_vp]),
    "dmnerf_skip_grid_dilate": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "dmnerf_skip_gather_samples": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_rows_scatter": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_int, c_vp]),
    "dmnerf_rows_gather": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_int, c_vp]),
    "dmnerf_label_cells": (c_int, [c_vp, c_i64, c_int, c_float, c_vp, c_vp]),
    "dmnerf_label_stats": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_skip_grid_from_labels": (c_int, [c_vp, c_i64, ctypes.POINTER(ctypes.c_uint32), c_vp, c_vp]),
    "dmnerf_label_components": (ctypes.c_int32, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "dmnerf_label_components_largest": (ctypes.c_int32, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_label_components_filter": (ctypes.c_int32, [c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_uint32), c_vp, c_vp, c_int, c_int,
                                               c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_label_trace": (c_int, [c_vp, ctypes.POINTER(c_float), ctypes.POINTER(c_float), ctypes.POINTER(c_float), ctypes.POINTER(c_int), c_int,
                                   c_vp, c_int, c_i64, ctypes.POINTER(ctypes.c_uint32), c_float, c_float, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_bake_cells": (c_int, [c_vp, c_i64, c_int, c_float, c_vp, c_vp, c_vp]),
    "dmnerf_baked_render": (c_int, [c_vp, c_vp, ctypes.POINTER(c_float), ctypes.POINTER(c_float), ctypes.POINTER(c_float), ctypes.POINTER(c_int),
                                    c_int, c_vp, c_int, c_i64, ctypes.POINTER(ctypes.c_uint32), c_float, c_float, c_float, c_vp, c_vp, c_vp, c_vp,
                                    c_vp, c_vp, c_vp]),
    "dmnerf_volume_edit": (ctypes.c_int32, [c_vp, c_vp, ctypes.POINTER(c_float), ctypes.POINTER(c_float), ctypes.POINTER(c_float), ctypes.POINTER(c_int),
                                   c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(VolumeEditEntry), c_int, c_int, c_vp, c_vp, c_vp,
                                   c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_field_edit_select": (ctypes.c_int32, [c_vp, ctypes.POINTER(c_float), ctypes.POINTER(c_float), ctypes.POINTER(c_int), c_int, c_int,
                                         ctypes.POINTER(VolumeEditEntry), c_int, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp,
                                         c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "dmnerf_field_edit_filter": (ctypes.c_int32, [c_vp, c_vp, c_i64, c_int, ctypes.POINTER(ctypes.c_uint32), c_int, c_vp, c_vp, c_vp]),
}

_lib = None


def load():
    """Load the shared library (idempotent).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C dm_nerf_amd/csrc`).  dm_nerf_amd has no CPU / eager fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.dmnerf_abi_version() != 8:
        raise RuntimeError("libdmnerf_hip.so ABI version mismatch")
    _lib = lib
    return lib


def last_error():
    return load().dmnerf_last_error().decode("utf-8", "replace")


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {last_error()}")


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu(*tensors):
    """Validate device / dtype / contiguity before handing raw pointers to the library."""
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("dm_nerf_amd runs on MI355X only: got a CPU tensor (there is no CPU fallback)")
        if not t.is_contiguous():
            raise RuntimeError("dm_nerf_amd: tensor must be contiguous")


def f32(t):
    """float32 + contiguous view/copy of a GPU tensor (plumbing)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def box_args(grid):
    """The box of a grid volume (anything with ``lo``, ``cell``, ``inv_cell [3]`` and ``dims``: ``field.SkipGrid`` / ``LabelGrid`` /
    ``BakedGrid``, ``editing.FieldEdit``) as the host arrays the entries take -> ``(lo, cell, inv_cell, dims)``, ctypes ``float[3]`` x 3
    and ``int[3]``."""
    f3 = lambda v: (c_float * 3)(*[float(x) for x in v])
    return f3(grid.lo), f3(grid.cell), f3(grid.inv_cell), (c_int * 3)(*grid.dims)


def _arg(a):
    """One argument as ctypes takes it: a tensor's / host array's address, a struct by reference, anything else (numbers,
    None = null, ``byref`` of a scalar, ctypes arrays) as it is.  No validation: that is the caller's."""
    if isinstance(a, torch.Tensor):
        return a.data_ptr()
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if isinstance(a, ctypes.Structure):
        return ctypes.byref(a)
    return a


def call(name, *args):
    """Host-only entry ``name`` (returns an int status, takes no stream); raises on a non-zero status."""
    check(getattr(load(), name)(*map(_arg, args)), name)


def launch(name, *args):
    """Entry ``name`` whose last C parameter is ``void* stream``: launched on the stream that is current NOW."""
    check(getattr(load(), name)(*map(_arg, args), stream()), name)
