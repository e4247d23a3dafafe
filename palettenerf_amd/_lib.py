"""ctypes binding of libpnr_hip.so -- the C ABI declared in include/pnr.h.

There is NO fallback: if the library is missing or a symbol is absent this module raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PNR_LIB_PATH") or os.path.join(_HERE, "libpnr_hip.so")   # PNR_LIB_PATH: an experiment build (palettenerf_amd.build --variant); still no fallback

_u32, _f32, _int, _ptr, _u64 = ctypes.c_uint32, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64

# name -> argtypes (restype is int unless listed in _RESTYPES); mirrors include/pnr.h one to one
SIGNATURES = {
    "pnr_abi_version": [],
    "pnr_set_option": [ctypes.c_char_p, _int],
    "pnr_error_string": [_int],
    "pnr_scan_scratch_bytes": [_u32],
    "pnr_near_far_from_aabb": [_ptr, _ptr, _ptr, _u32, _f32, _ptr, _ptr, _ptr],
    "pnr_sph_from_ray": [_ptr, _ptr, _f32, _u32, _ptr, _ptr],
    "pnr_morton3d": [_ptr, _u32, _ptr, _ptr],
    "pnr_morton3d_invert": [_ptr, _u32, _ptr, _ptr],
    "pnr_packbits": [_ptr, _u32, _f32, _ptr, _ptr],
    "pnr_march_rays_train": [_ptr, _ptr, _ptr, _f32, _f32, _u32, _u32, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                             _ptr, _ptr, _ptr],
    "pnr_composite_rays_train_forward": [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _f32, _ptr, _ptr, _ptr, _ptr],
    "pnr_composite_rays_train_backward": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _f32, _ptr, _ptr, _ptr],
    "pnr_composite_rays_train_norm_forward": [_ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _f32, _ptr, _ptr, _ptr, _ptr, _ptr],
    "pnr_composite_rays_train_norm_backward": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _f32, _ptr, _ptr,
                                               _ptr],
    "pnr_composite_rays_flex_train_forward": [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _f32, _ptr, _ptr],
    "pnr_composite_rays_flex_train_backward": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _f32, _ptr, _ptr],
    "pnr_spread_ray_to_sample": [_ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr],
    "pnr_march_rays": [_u32, _u32, _ptr, _ptr, _ptr, _ptr, _f32, _f32, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr],
    "pnr_composite_rays": [_u32, _u32, _f32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr],
    "pnr_composite_rays_flex": [_u32, _u32, _u32, _f32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr],
    "pnr_composite_rays_flex_multi": [_u32, _u32, _f32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr],
    "pnr_occupancy_mip_bytes": [_u32, _u32],
    "pnr_build_occupancy_mip": [_ptr, _u32, _u32, _f32, _ptr, _ptr],
    "pnr_march_rays_mip": [_u32, _u32, _ptr, _ptr, _ptr, _ptr, _f32, _f32, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr],
    "pnr_march_rays_fill": [_u32, _u32, _ptr, _ptr, _ptr, _ptr, _f32, _f32, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr],
    "pnr_march_rays_train_mip": [_ptr, _ptr, _ptr, _f32, _f32, _u32, _u32, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                 _ptr, _ptr, _ptr, _ptr, _ptr],
    "pnr_compact_alive": [_u32, _ptr, _ptr, _ptr, _ptr, _ptr],
    "pnr_grid_encode_forward": [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _u32, _f32, _u32, _ptr, _u32, _int, _int, _ptr],
    "pnr_grid_encode_forward_layout": [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _u32, _f32, _u32, _ptr, _u32, _int, _int, _int, _ptr],
    "pnr_grid_encode_forward_pair": [_ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _f32, _u32, _u32, _int, _ptr],
    "pnr_grid_encode_backward": [_ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _u32, _f32, _u32, _ptr, _ptr, _u32, _int, _int, _ptr],
    "pnr_nerf_field_packed_bytes": [],
    "pnr_nerf_field_pack": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _ptr],
    "pnr_nerf_field_forward": [_ptr, _ptr, _ptr, _u32, _ptr, _ptr, _int, _f32, _ptr],
    "pnr_nerf_density_forward": [_ptr, _ptr, _u32, _f32, _ptr, _ptr, _int, _f32, _ptr],
    "pnr_nerf_frame_workspace_bytes": [_u32],
    "pnr_nerf_render_frame": [_ptr, _ptr],
    "pnr_nerf_render_frame_submit": [_ptr, _ptr],
    "pnr_nerf_render_frame_finish": [_ptr, _ptr],
    "pnr_palette_field_packed_bytes": [_u32, _u32, _int],
    "pnr_palette_aux_channels": [_u32, _u32],
    "pnr_palette_field_pack": [_ptr, _ptr, _ptr],
    "pnr_palette_field_forward": [_ptr, _ptr],
    "pnr_palette_frame_workspace_bytes": [_u32, _u32, _u32, _int],
    "pnr_palette_render_frame": [_ptr, _ptr],
    "pnr_palette_render_frame_submit": [_ptr, _ptr],
    "pnr_palette_render_frame_finish": [_ptr, _ptr],
    "pnr_sh_encode_forward": [_ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr],
    "pnr_sh_encode_cat_forward": [_ptr, _ptr, _u32, _ptr, _u32, _u32, _ptr],
    "pnr_sigma_geo_cat_forward": [_ptr, _u32, _ptr, _u32, _u32, _ptr, _ptr, _ptr],
    "pnr_sigma_geo_cat_backward": [_ptr, _u32, _ptr, _ptr, _u32, _u32, _ptr, _ptr],
    "pnr_sh_encode_backward": [_ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr],
    "pnr_rgb_to_hsv": [_u32, _ptr, _ptr, _ptr],
    "pnr_hsv_to_rgb": [_u32, _ptr, _ptr, _ptr],
    "pnr_rgb_histogram": [_ptr, _ptr, _u32, _int, _ptr, _ptr, _ptr],
    "pnr_grid_backward_binned_workspace_bytes": [_u32, _u32, _u64],
    "pnr_grid_encode_backward_binned": [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _u32, _f32, _u32, _u32, _int, _u64, _ptr, _u64, _ptr],
    "pnr_linear_wgrad_workspace_bytes": [_u32, _u32, _u32],
    "pnr_linear_wgrad": [_ptr, _int, _ptr, _int, _u32, _u32, _u32, _ptr, _int, _ptr, _u64, _ptr],
    "pnr_mlp_packed_bytes": [_ptr],
    "pnr_mlp_pack": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr],
    "pnr_mlp_forward": [_ptr, _ptr, _ptr, _u32, _ptr, _ptr],
    "pnr_mlp_backward_workspace_bytes": [_ptr, _u32],
    "pnr_mlp_backward": [_ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _u64, _ptr],
    "pnr_mlp_forward_lm": [_ptr, _ptr, _ptr, _u32, _ptr, _u32, _ptr, _ptr],
    "pnr_mlp_backward_lm": [_ptr, _ptr, _ptr, _u32, _ptr, _ptr, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _u64, _ptr],
    "pnr_linear_bgrad": [_ptr, _int, _u32, _u32, _ptr, _int, _ptr, _u64, _ptr],
    "pnr_train_loss_workspace_bytes": [_u32],
    "pnr_train_loss_forward": [_ptr, _ptr],
    "pnr_train_loss_backward": [_ptr, _ptr],
    "pnr_palette_field_stages_aux": [_u32, _u32, _int],
    "pnr_interleave_tables": [_ptr, _ptr, _u64, _ptr, _ptr],
    "pnr_interleave_tables3": [_ptr, _ptr, _ptr, _u64, _ptr, _ptr],
    "pnr_interleave_tables3_half": [_ptr, _ptr, _ptr, _u64, _ptr, _ptr],
    "pnr_palette_train_shade_workspace_bytes": [_u32],
    "pnr_palette_train_shade_forward": [_u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr],
    "pnr_palette_train_shade_backward": [_u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u64, _ptr],
    "pnr_palette_smooth_points": [_ptr, _ptr, _f32, _u32, _ptr, _ptr],
    "pnr_palette_smooth_forward": [_u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _f32, _f32, _f32, _f32, _ptr, _ptr, _ptr],
    "pnr_palette_smooth_backward": [_u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr],
    "pnr_palette_heads_forward": [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr],
    "pnr_palette_heads_backward": [_ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr],
    "pnr_image_to_uint8": [_ptr, _u64, _int, _ptr, _ptr],
    "pnr_present_frame": [_ptr, _ptr],
    "pnr_adam_max_tensors": [],
    "pnr_adam_step": [_ptr, _u32, _ptr, _ptr],
    "pnr_grad_check": [_ptr, _u32, _ptr, _ptr],
    "pnr_adam_step_amp": [_ptr, _u32, _ptr, _u32, _ptr, _ptr],
    "pnr_ema_update": [_ptr, _u32, _f32, _ptr],
    "pnr_ema_swap": [_ptr, _u32, _ptr],
    "pnr_get_rays": [_ptr, _u32, _f32, _f32, _f32, _f32, _u32, _u32, _ptr, _u32, _ptr, _ptr, _ptr],
    "pnr_checksum": [_ptr, _ptr, _ptr, _u32, _ptr, _ptr],
    "pnr_occupancy_workspace_bytes": [_u32, _u32, _u32],
    "pnr_occupancy_samples": [_ptr],
    "pnr_occupancy_update": [_ptr, _ptr],
    "pnr_occupancy_begin": [_ptr, _ptr],
    "pnr_occupancy_points": [_ptr, _u32, _u32, _ptr, _ptr],
    "pnr_occupancy_scatter": [_ptr, _ptr, _ptr, _u32, _ptr],
    "pnr_occupancy_commit": [_ptr, _ptr],
    "pnr_mark_untrained_grid": [_ptr, _u32, _f32, _f32, _f32, _f32, _u32, _u32, _f32, _f32, _int, _ptr, _ptr, _ptr],
    "pnr_background_packed_bytes": [],
    "pnr_background_pack": [_ptr, _ptr, _ptr, _ptr],
    "pnr_background_forward": [_ptr, _ptr],
    "pnr_background_train_forward": [_ptr, _ptr],
    "pnr_background_backward_workspace_bytes": [_u32],
    "pnr_background_backward": [_ptr, _ptr],
    "pnr_train_loss_backward_bg": [_ptr, _ptr, _ptr],
    "pnr_launch_geometry": [ctypes.c_char_p, _u64, ctypes.POINTER(_u32), ctypes.POINTER(_u32)],
    "pnr_lattice_points": [_ptr, _ptr, _ptr, _u64, _u32, _ptr, _ptr],
    "pnr_lattice_density_workspace_bytes": [_u32],
    "pnr_lattice_density": [_ptr, _ptr],
    "pnr_mesh_case_triangles": [_u32, _ptr],
    "pnr_mesh_workspace_bytes": [_u32, _u32, _u32],
    "pnr_mesh_count": [_ptr, _u32, _u32, _u32, _f32, _ptr, _u64, _ptr, _ptr],
    "pnr_mesh_emit": [_ptr, _u32, _u32, _u32, _f32, _ptr, _u64, _ptr, _u32, _ptr, _u32, _ptr],
    "pnr_palette_sheets": [_ptr, _ptr],
    "pnr_frame_metrics_workspace_bytes": [_u32, _u32],
    "pnr_frame_metrics": [_ptr, _ptr],
    "pnr_train_batch": [_ptr, _ptr],
    "pnr_error_map_update": [_ptr, _u32, _ptr, _ptr, _ptr, _u32, _u32, _ptr],
    "pnr_stylizer_fit": [_ptr, _ptr],
    "pnr_density_gradient": [_ptr, _ptr],
    "pnr_mesh_vertex_record_bytes": [_int, _int, _u32],
    "pnr_mesh_vertex_records": [_ptr, _ptr],
    "pnr_extract_accumulate": [_ptr, _ptr],
    "pnr_extract_kmeans_workspace_bytes": [],
    "pnr_extract_kmeans": [_ptr, _ptr],
    "pnr_lut_weights": [_ptr, _ptr],
}
_RESTYPES = {"pnr_frame_metrics_workspace_bytes": _u64, "pnr_mesh_workspace_bytes": _u64, "pnr_lattice_density_workspace_bytes": _u64, "pnr_occupancy_workspace_bytes": _u64, "pnr_occupancy_samples": _u32, "pnr_adam_max_tensors": _u32, "pnr_error_string": ctypes.c_char_p, "pnr_scan_scratch_bytes": _u64, "pnr_nerf_field_packed_bytes": _u64, "pnr_occupancy_mip_bytes": _u64, "pnr_nerf_frame_workspace_bytes": _u64, "pnr_palette_field_packed_bytes": _u64, "pnr_palette_frame_workspace_bytes": _u64,
             "pnr_palette_aux_channels": _u32, "pnr_linear_wgrad_workspace_bytes": _u64, "pnr_grid_backward_binned_workspace_bytes": _u64,
             "pnr_palette_train_shade_workspace_bytes": _u64, "pnr_train_loss_workspace_bytes": _u64, "pnr_mlp_packed_bytes": _u64, "pnr_mlp_backward_workspace_bytes": _u64,
             "pnr_background_packed_bytes": _u64, "pnr_background_backward_workspace_bytes": _u64, "pnr_mesh_vertex_record_bytes": _u32, "pnr_extract_kmeans_workspace_bytes": _u64}

class AdamTensor(ctypes.Structure):
    """Mirror of `pnr_adam_tensor` (include/pnr.h)."""
    _fields_ = [("param", _ptr), ("grad", _ptr), ("exp_avg", _ptr), ("exp_avg_sq", _ptr), ("n", _u64)]


class AdamScalars(ctypes.Structure):
    """Mirror of `pnr_adam_scalars` (include/pnr.h)."""
    _fields_ = [(n, _f32) for n in ("one_minus_beta1", "beta2", "one_minus_beta2", "bias_correction2_sqrt", "eps", "neg_step_size", "inv_grad_scale")]


class AdamAmpCtl(ctypes.Structure):
    """Mirror of `pnr_adam_amp_ctl` (include/pnr.h)."""
    _fields_ = [("scale", _ptr), ("found_inf", _ptr), ("state", _ptr), ("skipped_base", ctypes.c_int32), ("parity", ctypes.c_int32)]


class EmaTensor(ctypes.Structure):
    """Mirror of `pnr_ema_tensor` (include/pnr.h)."""
    _fields_ = [("param", _ptr), ("shadow", _ptr), ("n", _u64)]


MLP_OUT_SIGMOID = 0x100   # PNR_MLP_OUT_SIGMOID


FLEX_MAX_MAPS = 8


class FlexMap(ctypes.Structure):
    """Mirror of `pnr_flex_map` (include/pnr.h)."""
    _fields_ = [("n_channel", _u32), ("input", _ptr), ("output", _ptr)]


class MlpDesc(ctypes.Structure):
    """Mirror of `pnr_mlp_desc` (include/pnr.h)."""
    _fields_ = [("n_layers", _u32), ("dims", _u32 * 4), ("activation", _int)]


class OccupancyArgs(ctypes.Structure):
    """Mirror of `pnr_occupancy_args` (include/pnr.h)."""
    _fields_ = [("C", _u32), ("H", _u32), ("bound", _f32), ("density_grid", _ptr), ("density_bitfield", _ptr), ("mip", _ptr), ("density_scale", _f32),
                ("decay", _f32), ("density_thresh", _f32), ("mode", _int), ("n_partial", _u32), ("noise", _ptr), ("coords", _ptr), ("occ_rand", _ptr),
                ("embeddings", _ptr), ("offsets", _ptr), ("num_levels", _u32), ("S", _f32), ("base_resolution", _u32), ("gridtype", _u32),
                ("packed_sigma_net", _ptr), ("workspace", _ptr), ("workspace_bytes", _u64), ("state", _ptr), ("points_out", _ptr)]


class LatticeDensityArgs(ctypes.Structure):
    """Mirror of `pnr_lattice_density_args` (include/pnr.h)."""
    _fields_ = [("box_min", _f32 * 3), ("box_max", _f32 * 3), ("n", _u32 * 3), ("bound", _f32), ("embeddings", _ptr), ("offsets", _ptr),
                ("num_levels", _u32), ("S", _f32), ("base_resolution", _u32), ("gridtype", _u32), ("packed_sigma_net", _ptr), ("workspace", _ptr),
                ("workspace_bytes", _u64), ("u", _ptr)]


class DensityGradientArgs(ctypes.Structure):
    """Mirror of `pnr_density_gradient_args` (include/pnr.h)."""
    _fields_ = [("points", _ptr), ("n", _u32), ("bound", _f32), ("embeddings", _ptr), ("offsets", _ptr), ("num_levels", _u32), ("S", _f32),
                ("base_resolution", _u32), ("gridtype", _u32), ("sigma0", _ptr), ("sigma1", _ptr), ("logit", _ptr), ("grad", _ptr), ("normal", _ptr)]


class VertexRecordsArgs(ctypes.Structure):
    """Mirror of `pnr_vertex_records_args` (include/pnr.h)."""
    _fields_ = [("vertices", _ptr), ("nv", _u32), ("box_min", _f32 * 3), ("box_max", _f32 * 3), ("n", _u32 * 3), ("normal", _ptr), ("rgb", _ptr),
                ("linear_to_srgb", _int), ("extra", _ptr), ("extra_channels", _u32), ("extra_stride", _u32), ("world", _ptr), ("records", _ptr)]


class NerfFrameArgs(ctypes.Structure):
    """Mirror of `pnr_nerf_frame_args` (include/pnr.h)."""
    _fields_ = [("N", _u32), ("rays_o", _ptr), ("rays_d", _ptr), ("nears", _ptr), ("fars", _ptr), ("bitfield", _ptr), ("mip", _ptr), ("bound", _f32),
                ("C", _u32), ("H", _u32), ("dt_gamma", _f32), ("max_steps", _u32), ("T_thresh", _f32), ("embeddings", _ptr), ("offsets", _ptr),
                ("num_levels", _u32), ("S", _f32), ("base_resolution", _u32), ("gridtype", _u32), ("packed_weights", _ptr), ("field_precision", _int), ("density_scale", _f32),
                ("weights_sum", _ptr), ("depth", _ptr), ("image", _ptr), ("workspace", _ptr), ("workspace_bytes", _u64), ("stats", _ptr), ("kernel_ms", _ptr), ("ray_order", _ptr),
                ("finish", _int), ("bg_color", _f32 * 3), ("bg_map", _ptr), ("table_dtype", _int), ("enc_scale", _f32 * 3), ("watch_overflow", _int),
                ("aabb", _ptr), ("min_near", _f32), ("depth_raw", _ptr), ("noises", _ptr)]


MAX_BASIS, MAX_CLIP = 10, 32   # PNR_MAX_BASIS, PNR_MAX_CLIP


class PaletteEdit(ctypes.Structure):
    """Mirror of `pnr_palette_edit` (include/pnr.h)."""
    _fields_ = [("mode", _int), ("delta_hsv", (_f32 * 3) * MAX_BASIS), ("has_mean_xyz", _int), ("mean_xyz", _f32 * 3), ("std_xyz", _f32),
                ("has_mean_clip", _int), ("mean_clip", _f32 * MAX_CLIP), ("std_clip", _f32), ("weight_mode", _int),
                ("dI", _f32 * MAX_BASIS), ("dP", (_f32 * 3) * MAX_BASIS), ("ddelta", ((_f32 * 3) * 3) * MAX_BASIS)]


class PaletteFrameArgs(ctypes.Structure):
    """Mirror of `pnr_palette_frame_args` (include/pnr.h)."""
    _fields_ = [("base", NerfFrameArgs), ("embeddings_palette", _ptr), ("embeddings_clip", _ptr),
                ("num_basis", _u32), ("clip_dim", _u32), ("pred_clip", _int), ("offsets_weight", _f32), ("view_dep_weight", _f32), ("aux_map", _ptr), ("embeddings_pair", _ptr), ("embeddings_triple", _ptr),
                ("edit", _ptr)]


class PresentArgs(ctypes.Structure):
    """Mirror of `pnr_present_args` (include/pnr.h)."""
    _fields_ = ([(n, _u32) for n in ("src_h", "src_w", "dst_h", "dst_w")]
                + [(n, _ptr) for n in ("image", "depth", "rays_o", "rays_d", "depth_origin", "clip_feat")]
                + [("clip_dim", _u32), ("clip_stride", _u32), ("linear_to_srgb", _int)]
                + [(n, _ptr) for n in ("out_image", "out_depth", "out_xyz", "out_clip", "accum")] + [("spp", _u32)])


class PaletteWeights(ctypes.Structure):
    """Mirror of `pnr_palette_weights` (include/pnr.h)."""
    _fields_ = [(n, _ptr) for n in ("sigma0", "sigma1", "diff0", "diff1", "diff2", "color0", "color1", "color2", "basis0", "basis1",
                                    "offsets_radiance", "omega", "clip0", "clip1", "basis_color", "or_bias")] + [("num_basis", _u32), ("clip_dim", _u32), ("pred_clip", _int), ("precision", _int)]


class PaletteFieldArgs(ctypes.Structure):
    """Mirror of `pnr_palette_field_args` (include/pnr.h)."""
    _fields_ = [("ctl", _ptr), ("B", _u32), ("enc", _ptr), ("enc_palette", _ptr), ("enc_clip", _ptr), ("level_stride", _u32), ("dirs", _ptr),
                ("deltas", _ptr), ("packed", _ptr), ("num_basis", _u32), ("clip_dim", _u32),
                ("pred_clip", _int), ("density_scale", _f32), ("offsets_weight", _f32), ("view_dep_weight", _f32), ("aux_stride", _u32),
                ("sigmas", _ptr), ("rgbs", _ptr), ("aux", _ptr), ("rays_alive", _ptr), ("weights_sum", _ptr), ("aux_map", _ptr), ("T_thresh", _f32),
                ("precision", _int), ("edit", _ptr), ("xyzs", _ptr), ("edit_device", _ptr), ("enc_scale", _f32 * 3), ("overflow_flag", _ptr), ("tile_counter", _ptr),
                ("rays_t", _ptr), ("weights_sum_rw", _ptr), ("depth", _ptr), ("image", _ptr), ("rays_alive_rw", _ptr), ("counts_cur", _ptr)]   # frame loop only: leave NULL


class TrainLossArgs(ctypes.Structure):
    """Mirror of `pnr_train_loss_args` (include/pnr.h)."""
    _fields_ = ([(n, _u32) for n in ("N", "n_channel", "num_basis", "clip_dim")]
                + [(n, _ptr) for n in ("weights_sum", "depth_raw", "image_raw", "all_map", "nears", "fars", "bg_color")]
                + [("bg_const", _f32), ("bg_mode", ctypes.c_int32)]
                + [(n, _ptr) for n in ("gt_rgb", "gt_clip", "gt_weights", "basis_color", "basis_color_origin")]
                + [(n, _f32) for n in ("lambda_sparsity", "lambda_offsets", "lambda_view_dep", "lambda_smooth", "lambda_weight", "lambda_palette")]
                + [(n, _ptr) for n in ("image", "depth", "direct_rgb", "loss_ray", "terms", "grad_loss", "grad_weights_sum", "grad_image_raw",
                                       "grad_all_map", "grad_basis_color", "workspace")]
                + [("workspace_bytes", _u64)])


TRAIN_LOSS_TERMS = 10   # PNR_TRAIN_LOSS_TERMS


class BackgroundArgs(ctypes.Structure):
    """Mirror of `pnr_background_args` (include/pnr.h, ABI 10)."""
    _fields_ = [("N", _u32), ("rays_o", _ptr), ("rays_d", _ptr), ("radius", _f32), ("coords_in", _ptr), ("embeddings", _ptr), ("table_dtype", _int),
                ("offsets", _ptr), ("table_rows", _u32), ("num_levels", _u32), ("level_dim", _u32), ("S", _f32), ("H", _u32), ("gridtype", _u32),
                ("align_corners", _int), ("sh_degree", _u32), ("num_layers", _u32), ("hidden_dim", _u32), ("packed", _ptr), ("out", _ptr),
                ("coords_out", _ptr)]


class BackgroundTrainArgs(ctypes.Structure):
    """Mirror of `pnr_background_train_args` (include/pnr.h)."""
    _fields_ = [("N", _u32), ("rays_o", _ptr), ("rays_d", _ptr), ("radius", _f32), ("coords_in", _ptr), ("embeddings", _ptr), ("table_dtype", _int),
                ("offsets", _ptr), ("table_rows", _u32), ("num_levels", _u32), ("level_dim", _u32), ("S", _f32), ("H", _u32), ("gridtype", _u32),
                ("align_corners", _int), ("sh_degree", _u32), ("num_layers", _u32), ("hidden_dim", _u32), ("w0", _ptr), ("w1", _ptr), ("out", _ptr),
                ("coords_out", _ptr), ("grad_rgb", _ptr), ("grad_w0", _ptr), ("grad_w1", _ptr), ("grad_table", _ptr), ("workspace", _ptr),
                ("workspace_bytes", _u64)]


SHEET_MAX_BASIS = 8   # PNR_SHEET_MAX_BASIS
METRIC_MSE, METRIC_PSNR, METRIC_SSIM, METRIC_SPARSITY, METRIC_TV = 1, 2, 4, 8, 16   # PNR_METRIC_*


class SheetArgs(ctypes.Structure):
    """Mirror of `pnr_sheet_args` (include/pnr.h)."""
    _fields_ = ([("H", _u32), ("W", _u32), ("num_basis", _u32), ("linear_to_srgb", _int)]
                + [(n, _ptr) for n in ("image", "depth", "view_dep_rgb", "direct_rgb", "basis_rgb", "unscaled_basis_rgb", "basis_acc", "gt_weights", "basis_color")]
                + [(n, _u32) for n in ("image_stride", "depth_stride", "view_dep_stride", "direct_stride", "basis_rgb_stride", "unscaled_stride",
                                       "basis_acc_stride", "gt_weights_stride")]
                + [(n, _ptr) for n in ("out_rgb", "out_depth", "out_view_dep", "out_direct", "out_basis_img", "out_unscaled_basis_img", "out_basis_acc",
                                       "out_weights_guide", "out_basis_color")])


class MetricsArgs(ctypes.Structure):
    """Mirror of `pnr_metrics_args` (include/pnr.h)."""
    _fields_ = [("H", _u32), ("W", _u32), ("pred", _ptr), ("pred_stride", _u32), ("truth", _ptr), ("truth_channels", _u32), ("srgb_to_linear_truth", _int),
                ("basis_acc", _ptr), ("basis_acc_stride", _u32), ("num_basis", _u32), ("want", _u32), ("truth_rgb_out", _ptr), ("totals", _ptr),
                ("frame_out", _ptr), ("workspace", _ptr), ("workspace_bytes", _u64)]


IMAGE_FP32, IMAGE_FP16, IMAGE_UINT8 = 0, 1, 2   # PNR_IMAGE_*


class TrainBatchArgs(ctypes.Structure):
    """Mirror of `pnr_train_batch_args` (include/pnr.h)."""
    _fields_ = ([(n, _u32) for n in ("V", "H", "W", "C")]
                + [("images", _ptr), ("image_format", _int), ("feat_images", _ptr), ("feat_format", _int), ("D", _u32), ("poses", _ptr)]
                + [(n, _f32) for n in ("fx", "fy", "cx", "cy")]
                + [("view_index", _ptr), ("inds", _ptr), ("B", _u32), ("N", _u32), ("bg_mode", _int), ("bg_const", _f32), ("bg_color", _ptr),
                   ("hist_weights", _ptr)]
                + [(n, _u32) for n in ("num_basis", "Sr", "Sg", "Sb")] + [("hist_stride", _u64 * 4), ("srgb_to_linear", _int)]
                + [(n, _ptr) for n in ("rays_o", "rays_d", "pixels", "gt_rgb", "gt_weights", "gt_clip")])


STYLIZER_MIN_BASIS, STYLIZER_MAX_POINTS, STYLIZER_MAX_ITERS = 4, 512, 10000   # PNR_STYLIZER_MAX_POINTS, PNR_STYLIZER_MAX_ITERS


class StylizerFitArgs(ctypes.Structure):
    """Mirror of `pnr_stylizer_fit_args` (include/pnr.h)."""
    _fields_ = ([(n, _u32) for n in ("M", "num_basis", "iters")]
                + [(n, _ptr) for n in ("radiance", "omega", "offsets", "palette", "target", "view_dep", "dI", "dP", "ddelta", "mom_dI", "mom_dP",
                                       "mom_ddelta")]
                + [("has_momentum", _int), ("lr", _ptr), ("momentum", _f32), ("lambda_arap", _f32), ("trace", _ptr)])


EXTRACT_COARSE_BINS, EXTRACT_FINE_BINS, EXTRACT_MAX_K = 512, 32768, 128   # PNR_EXTRACT_*
EXTRACT_STOP = ("max_iter", "labels", "shift")                             # PNR_EXTRACT_STOP_CAP, _LABELS, _SHIFT
EXTRACT_OK, EXTRACT_EMPTIED, EXTRACT_NO_CENTER, EXTRACT_TOO_MANY, EXTRACT_FEW_POINTS = 0, 1, 2, 3, 4


class ExtractAccumulateArgs(ctypes.Structure):
    """Mirror of `pnr_extract_accumulate_args` (include/pnr.h)."""
    _fields_ = [("H", _u32), ("W", _u32), ("weights_sum", _ptr), ("pixels", _ptr), ("image_format", _int), ("channels", _u32),
                ("row_stride_bytes", _u64), ("linear", _int), ("thresh", _f32), ("counts_coarse", _ptr), ("counts_fine", _ptr), ("total", _ptr)]


class ExtractKmeansArgs(ctypes.Structure):
    """Mirror of `pnr_extract_kmeans_args` (include/pnr.h)."""
    _fields_ = [("counts_coarse", _ptr), ("counts_fine", _ptr), ("total", _ptr), ("tau", ctypes.c_double), ("tol", ctypes.c_double), ("max_iter", _u32),
                ("workspace", _ptr), ("workspace_bytes", _u64), ("centers", _ptr), ("center_weights", _ptr), ("info", _ptr), ("labels", _ptr)]


LUT_MIN_M, LUT_MAX_M, LUT_MAX_FACES = 4, 16, 28                             # PNR_LUT_*
LUT_POINTS_BINS, LUT_POINTS_FP32, LUT_POINTS_FP64 = 0, 1, 2
LUT_OK, LUT_FLAT, LUT_COPLANAR = 0, 1, 2


class LutWeightsArgs(ctypes.Structure):
    """Mirror of `pnr_lut_weights_args` (include/pnr.h)."""
    _fields_ = [("palette", _ptr), ("M", _u32), ("points", _ptr), ("points_format", _int), ("point_stride", _u64), ("N", _u32),
                ("normalize_input", _int), ("weights64", _ptr), ("lut32", _ptr), ("info", _ptr)]


# include/pnr_hull.h: the hull simplification.  A header and a table of its own beside include/pnr.h and SIGNATURES; load() binds both.
HULL_SIGNATURES = {
    "pnr_hull_simplify": [_ptr, _ptr],
}
HULL_MAX_M, HULL_MAX_RELATED = 16, 64                                       # PNR_HULL_*
HULL_OK, HULL_COPLANAR, HULL_FLAT, HULL_DENSE = 0, 1, 2, 3
HULL_STOP = ("none", "error", "target", "unchanged", "four")                # PNR_HULL_STOP_NONE, _ERROR, _TARGET, _UNCHANGED, _FOUR
HULL_ERROR_NONE, HULL_ERROR_FAIL = -1.0, -2.0                               # PNR_HULL_ERROR_*


class HullSimplifyArgs(ctypes.Structure):
    """Mirror of `pnr_hull_simplify_args` (include/pnr_hull.h)."""
    _fields_ = [("centers", _ptr), ("center_weights", _ptr), ("K", _u32), ("error_thres", ctypes.c_double), ("target_size", _u32),
                ("palette", _ptr), ("info", _ptr), ("errors", _ptr), ("trace", _ptr), ("vertices", _ptr)]


# include/pnr_distortion.h: the distortion loss on the ragged training rays.  A header and a table of its own, as the hull's.
DISTORTION_SIGNATURES = {
    "pnr_distortion_forward": [_ptr, _ptr, _ptr, _u32, _u32, _f32, _ptr, _ptr, _ptr, _ptr],
    "pnr_distortion_backward": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _f32, _ptr, _ptr],
}


_lib = None


def load():
    """Load the HIP library; raises RuntimeError (never falls back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"palettenerf_amd: {LIB_PATH} is missing. Build it with `python -m palettenerf_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU or PyTorch fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in (*SIGNATURES.items(), *HULL_SIGNATURES.items(), *DISTORTION_SIGNATURES.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"palettenerf_amd: symbol {name} missing from {LIB_PATH}; rebuild it") from e
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, _int)
    _lib = lib
    return lib


def check(rc, what):
    """Turn a non-zero C-ABI return into RuntimeError (the reference raises RuntimeError via TORCH_CHECK)."""
    if rc != 0:
        msg = load().pnr_error_string(rc)
        raise RuntimeError(f"{what}: {msg.decode() if msg else rc}")


_FN = {}     # name -> the loaded entry point (a getattr on the CDLL per call is a dict miss + a descriptor each time)


def call(name, *args):
    fn = _FN.get(name)
    if fn is None:
        fn = _FN[name] = getattr(load(), name)
    rc = fn(*args)
    if rc:
        check(rc, name)


def launch_geometry(entry, rows):
    """(workgroups, rows_per_trip) of a capped-grid entry for `rows` rows (pnr_launch_geometry, host only): a workgroup takes a second trip through
    its tile loop iff rows > workgroups * rows_per_trip."""
    wg, rpt = _u32(0), _u32(0)
    call("pnr_launch_geometry", entry.encode(), int(rows), ctypes.byref(wg), ctypes.byref(rpt))
    return wg.value, rpt.value
