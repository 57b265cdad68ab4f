"""ctypes binding of librcn.so (the C ABI declared in include/rcn.h).

The HIP library IS the product: if it is missing or cannot be loaded this module raises --
there is no CPU fallback anywhere in reconstructor_amd.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("RCN_LIB", os.path.join(_HERE, "librcn.so"))   # RCN_LIB: A/B another build of the same ABI

RCN_OK = 0
ERRORS = {-1: "RCN_ERR_ARG", -2: "RCN_ERR_HIP", -3: "RCN_ERR_NO_DEVICE",
          -4: "RCN_ERR_UNSUPPORTED", -5: "RCN_ERR_NOT_FOUND", -6: "RCN_ERR_NUMERIC",
          -7: "RCN_ERR_COMM", -8: "RCN_ERR_IO"}

# every symbol include/rcn.h declares (tests check the library exports exactly these)
SYMBOLS = [
    "rcn_create", "rcn_destroy", "rcn_last_error", "rcn_version", "rcn_set_stream",
    "rcn_synchronize", "rcn_desc_upload", "rcn_desc_upload_device", "rcn_desc_upload_batch_device", "rcn_desc_upload_batch", "rcn_desc_remove", "rcn_desc_sample_device", "rcn_desc_sample_errors", "rcn_desc_sample_batch_device", "rcn_desc_clear",
    "rcn_desc_count", "rcn_match_pair", "rcn_match_grid", "rcn_match_grid_device",
    "rcn_match_last_stats", "rcn_match_profile", "rcn_match_set_workspace_rows", "rcn_ba_default_options", "rcn_ba_solve", "rcn_ba_solve_robust", "rcn_ba_solve_constant", "rcn_ba_solve_tied", "rcn_ba_factor_plan",
    "rcn_landmark_validity", "rcn_landmark_validity_device",
    "rcn_fmat_filter", "rcn_fmat_filter_grid", "rcn_fmat_filter_grid_device",
    "rcn_coords_upload", "rcn_coords_upload_batch", "rcn_coords_clear", "rcn_match_table_filter_device",
    "rcn_host_alloc", "rcn_host_free", "rcn_match_compact_begin", "rcn_match_compact_wait",
    "rcn_shard_owned_images", "rcn_shard_pair_count", "rcn_shard_pairs", "rcn_shard_unique_id",
    "rcn_shard_create", "rcn_shard_destroy", "rcn_shard_ctx", "rcn_shard_reserve", "rcn_shard_put_image", "rcn_shard_exchange",
    "rcn_shard_match", "rcn_shard_lists", "rcn_shard_info", "rcn_device_count",
    "rcn_shard_fail", "rcn_shard_set_timeout", "rcn_shard_gather_lists", "rcn_shard_merge_lists", "rcn_shard_profile", "rcn_shard_profile_read", "rcn_shard_filter", "rcn_match_grid_filtered",
    "rcn_ba_session_create", "rcn_ba_session_destroy", "rcn_ba_session_add_camera", "rcn_ba_session_cameras",
    "rcn_ba_session_add_points", "rcn_ba_session_add_observations", "rcn_ba_session_counts", "rcn_ba_session_graph",
    "rcn_ba_session_solve", "rcn_ba_session_set_loss", "rcn_ba_session_set_groups", "rcn_ba_session_loss_report", "rcn_ba_session_read_points", "rcn_ba_session_points_device", "rcn_ba_session_validity",
    "rcn_ba_session_remove_outliers", "rcn_ba_session_triangulate",
    "rcn_ba_session_solve_local", "rcn_ba_session_covisible", "rcn_ba_session_local_seconds",
    "rcn_triangulate", "rcn_triangulate_device",
    "rcn_match_lists_upload", "rcn_match_lists_clear", "rcn_corr_set_workspace_bytes", "rcn_corr_2d3d", "rcn_corr_2d3d_device",
    "rcn_landmark_attach", "rcn_ba_session_attach",
    "rcn_landmark_ids_reset", "rcn_landmark_ids_set", "rcn_landmark_ids_read", "rcn_new_view_tracks_device",
    "rcn_new_view_triangulate_device", "rcn_ba_session_grow_view",
    "rcn_pnp_default_options", "rcn_pnp_ransac", "rcn_pnp_ransac_device", "rcn_ba_session_pnp",
    "rcn_twoview_default_options", "rcn_twoview_init", "rcn_twoview_init_device", "rcn_pose34_to_pose6", "rcn_ba_session_init_pair",
    "rcn_homography_default_options", "rcn_homography_ransac", "rcn_homography_ransac_device",
    "rcn_twoview_geometry_default_options", "rcn_twoview_geometry", "rcn_twoview_geometry_device",
    "rcn_kp_detect_device", "rcn_kp_nms_device",
    "rcn_sg_default_options", "rcn_sg_scores_device", "rcn_sg_assign_device", "rcn_sg_match_device", "rcn_sg_set_chunk_bytes",
    "rcn_sg_net_create", "rcn_sg_net_destroy", "rcn_sg_net_set_chunk_pairs", "rcn_sg_net_forward_device", "rcn_sg_net_match_device",
    "rcn_sp_net_create", "rcn_sp_net_destroy", "rcn_sp_net_set_chunk_images", "rcn_sp_net_forward_device", "rcn_sp_net_detect_device",
    "rcn_sift_default_options", "rcn_sift_layout", "rcn_sift_set_chunk_images", "rcn_sift_pyramid_device", "rcn_sift_candidates_device", "rcn_sift_detect_device",
    "rcn_sift_describe_device", "rcn_sift_detect_and_compute_device",
    "rcn_orb_default_options", "rcn_orb_default_pattern", "rcn_orb_layout", "rcn_orb_set_chunk_images", "rcn_orb_pyramid_device", "rcn_orb_fast_device",
    "rcn_orb_detect_device", "rcn_orb_describe_device", "rcn_orb_detect_and_compute_device",
    "rcn_bits_upload", "rcn_bits_upload_batch_device", "rcn_bits_remove", "rcn_bits_clear", "rcn_bits_count",
    "rcn_match_pair_hamming", "rcn_match_grid_hamming", "rcn_match_grid_hamming_device", "rcn_hamming_knn2_device",
    "rcn_guided_default_options", "rcn_match_guided_device", "rcn_match_guided", "rcn_match_pair_guided", "rcn_guided_knn2_device",
    "rcn_match_table_filter_model_device", "rcn_match_grid_guided",
    "rcn_tracks_default_options", "rcn_tracks_layout", "rcn_tracks_build_device", "rcn_tracks_build", "rcn_tracks_last_phase_ms",
    "rcn_retr_default_options", "rcn_retr_codebook_train_device", "rcn_retr_codebook_create", "rcn_retr_codebook_read", "rcn_retr_codebook_destroy",
    "rcn_retr_assign_device", "rcn_retr_encode_device", "rcn_retr_similarity_device", "rcn_retr_topk_device", "rcn_retr_pairs_device", "rcn_retr_image_pairs",
    "rcn_img_reshape_size", "rcn_img_resize_tables", "rcn_img_default_options", "rcn_img_prepare_plan", "rcn_img_prepare_device",
    "rcn_feat_colors_device", "rcn_landmark_colors_device", "rcn_cloud_vertices_device", "rcn_cloud_write_ply",
    "rcn_mvs_default_options", "rcn_mvs_layout", "rcn_mvs_inv_depths", "rcn_mvs_homographies", "rcn_img_undistort_device",
    "rcn_mvs_sweep_device", "rcn_mvs_consistency_device", "rcn_mvs_fuse_device", "rcn_ba_session_mvs_views",
    "rcn_store_save", "rcn_store_open", "rcn_store_contents_of", "rcn_store_close", "rcn_store_upload",
]
SHARD_ID_BYTES = 128


class RcnError(RuntimeError):
    def __init__(self, code, text=""):
        self.code = code
        super().__init__("%s (%d)%s" % (ERRORS.get(code, "RCN_ERR"), code, ": " + text if text else ""))


class MatchStats(C.Structure):
    _fields_ = [("rows_total", C.c_int64), ("rows_reranked", C.c_int64), ("rows_exact_fallback", C.c_int64),
                ("pair_distances", C.c_int64), ("err_bound_d2", C.c_double),
                ("used_mfma_path", C.c_int32), ("profiled_calls", C.c_int32),
                ("coarse_ms", C.c_double), ("rerank_ms", C.c_double), ("unique_ms", C.c_double),
                ("rows_brute_force", C.c_int64), ("chunks", C.c_int32), ("coarse_launches", C.c_int32),
                ("coarse_dtype", C.c_int32), ("reserved", C.c_int32)]


class ShardStats(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("n_images", C.c_int32), ("images_per_rank", C.c_int32),
                ("n_pairs", C.c_int64), ("exchange_bytes_f16", C.c_int64), ("exchange_bytes_f32", C.c_int64),
                ("comm_ranks", C.c_int32), ("reserved", C.c_int32)]


class ShardTimes(C.Structure):
    _fields_ = [("exchanges", C.c_int32), ("matches", C.c_int32), ("exchange_ms", C.c_double),
                ("f32_gather_ms", C.c_double), ("match_ms", C.c_double)]


class StoreContents(C.Structure):
    _fields_ = [("n_images", C.c_int32), ("D", C.c_int32), ("has_coords", C.c_int32), ("n_pairs", C.c_int32),
                ("img_ids", C.c_void_p), ("img_K", C.c_void_p), ("desc", C.c_void_p), ("coords", C.c_void_p),
                ("pairs", C.c_void_p), ("offsets", C.c_void_p), ("qt", C.c_void_p)]


class BaProblem(C.Structure):
    _fields_ = [("n_cams", C.c_int32), ("n_points", C.c_int32), ("n_obs", C.c_int32),
                ("reserved", C.c_int32),
                ("poses", C.c_void_p), ("intrinsics", C.c_void_p), ("points", C.c_void_p),
                ("obs_uv", C.c_void_p), ("obs_cam", C.c_void_p), ("obs_pt", C.c_void_p)]


class LandmarkProblem(C.Structure):
    _fields_ = [("n_cams", C.c_int32), ("n_points", C.c_int32), ("n_obs", C.c_int32),
                ("reserved", C.c_int32),
                ("poses34", C.c_void_p), ("intrinsics", C.c_void_p), ("points", C.c_void_p),
                ("pt_off", C.c_void_p), ("obs_cam", C.c_void_p), ("obs_xy", C.c_void_p)]


class TriangulationProblem(C.Structure):
    _fields_ = [("n_cams", C.c_int32), ("n_tracks", C.c_int32), ("n_obs", C.c_int32),
                ("reserved", C.c_int32),
                ("poses34", C.c_void_p), ("intrinsics", C.c_void_p),
                ("trk_off", C.c_void_p), ("obs_cam", C.c_void_p), ("obs_xy", C.c_void_p)]


class PnpOptions(C.Structure):
    _fields_ = [("max_projection_error", C.c_double), ("confidence", C.c_double), ("max_iterations", C.c_int32),
                ("refine_iterations", C.c_int32)]


class HomographyOptions(C.Structure):
    _fields_ = [("threshold", C.c_double), ("confidence", C.c_double), ("max_iterations", C.c_int32), ("reserved", C.c_int32)]


class TwoViewGeometryOptions(C.Structure):
    _fields_ = [("max_h_ratio", C.c_double), ("min_angle", C.c_double), ("min_inliers", C.c_int32), ("top_m", C.c_int32)]


class TwoViewOptions(C.Structure):
    _fields_ = [("threshold", C.c_double), ("confidence", C.c_double), ("distance_threshold", C.c_double),
                ("max_iterations", C.c_int32), ("reserved", C.c_int32)]


class SgOptions(C.Structure):
    _fields_ = [("alpha", C.c_double), ("match_threshold", C.c_double), ("score_threshold", C.c_double),
                ("iterations", C.c_int32), ("path", C.c_int32)]


class SiftOptions(C.Structure):
    _fields_ = [("n_octave_layers", C.c_int32), ("reserved", C.c_int32), ("contrast_threshold", C.c_double),
                ("edge_threshold", C.c_double), ("sigma", C.c_double)]


class SiftLayout(C.Structure):
    _fields_ = [("n_octaves", C.c_int32), ("n_layers", C.c_int32), ("base_taps", C.c_int32), ("reserved", C.c_int32),
                ("base_sigma", C.c_double), ("oct_h", C.c_int32 * 16), ("oct_w", C.c_int32 * 16),
                ("layer_sigma", C.c_double * 8), ("layer_taps", C.c_int32 * 8), ("layer_offset", (C.c_int64 * 8) * 16),
                ("floats_per_image", C.c_int64)]


class OrbOptions(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("nlevels", C.c_int32), ("edge_threshold", C.c_int32), ("fast_threshold", C.c_int32),
                ("scale_factor", C.c_double), ("pattern", C.c_void_p)]


class OrbLayout(C.Structure):
    _fields_ = [("n_levels", C.c_int32), ("reserved", C.c_int32), ("level_h", C.c_int32 * 16), ("level_w", C.c_int32 * 16),
                ("quota", C.c_int32 * 16), ("active", C.c_int32 * 16), ("scale", C.c_float * 16), ("level_offset", C.c_int64 * 16),
                ("bytes_per_image", C.c_int64)]


class ImgOptions(C.Structure):
    _fields_ = [("order", C.c_int32), ("gray_bits", C.c_int32)]


class GuidedOptions(C.Structure):
    _fields_ = [("ratio", C.c_float), ("max_error_px", C.c_float), ("max_distance", C.c_float), ("cross_check", C.c_int32)]


class TracksOptions(C.Structure):
    _fields_ = [("min_length", C.c_int32), ("max_length", C.c_int32), ("conflict", C.c_int32), ("reserved", C.c_int32)]


class MvsOptions(C.Structure):
    _fields_ = [("radius", C.c_int32), ("min_sources", C.c_int32), ("min_consistent", C.c_int32), ("stride", C.c_int32),
                ("max_cost", C.c_double), ("rel_tol", C.c_double)]


class MvsSizes(C.Structure):
    _fields_ = [("tile", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32), ("lds_bytes", C.c_int32),
                ("pixels", C.c_int64), ("h_doubles", C.c_int64), ("samples", C.c_int64)]


class RetrOptions(C.Structure):
    _fields_ = [("n_centroids", C.c_int32), ("iterations", C.c_int32), ("train_row_stride", C.c_int32), ("top_k", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class BaOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("intrinsics_mode", C.c_int32),
                ("fix_cam0_pose", C.c_int32), ("fix_cam1_translation", C.c_int32),
                ("focal_upper_bound", C.c_double),
                ("initial_trust_region_radius", C.c_double),
                ("max_trust_region_radius", C.c_double),
                ("min_trust_region_radius", C.c_double),
                ("min_relative_decrease", C.c_double),
                ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double),
                ("max_consecutive_invalid_steps", C.c_int32), ("jacobi_scaling", C.c_int32)]


class BaSummary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("initial_rms_px", C.c_double), ("final_rms_px", C.c_double),
                ("iterations", C.c_int32), ("successful_steps", C.c_int32),
                ("unsuccessful_steps", C.c_int32), ("invalid_steps", C.c_int32),
                ("termination", C.c_int32), ("line_search_backtracks", C.c_int32),
                ("bound_projections", C.c_int32), ("reduced_dim", C.c_int32),
                ("pair_lists_reused", C.c_int32), ("reserved", C.c_int32),
                ("solve_seconds", C.c_double), ("schur_seconds", C.c_double),
                ("cholesky_seconds", C.c_double), ("trisolve_seconds", C.c_double),
                ("cost_trace", C.c_double * 160),
                ("jacobian_seconds", C.c_double), ("jacobian_evals", C.c_int32), ("factor_schedule", C.c_int32)]


class BaLoss(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("scale", C.c_double)]


class BaLossReport(C.Structure):
    _fields_ = [("n_obs", C.c_int64), ("n_beyond_scale", C.c_int64), ("plain_rms_px", C.c_double), ("max_residual_px", C.c_double)]


_LIB = None


def load():
    """Load librcn.so.  torch (when used in the same process) must be imported first so that
    both share one HIP runtime (same SONAME libamdhip64.so.7); callers in this package do so."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(SO_PATH):
        raise ImportError(
            "reconstructor_amd/librcn.so is missing: run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    try:
        import torch  # noqa: F401  -- FIRST: torch ships its own ROCm runtime + RCCL under the same SONAMEs; whichever
    except ImportError:             # copy is mapped first serves both, and two copies in one process corrupt the heap at exit
        pass
    L = C.CDLL(SO_PATH, mode=C.RTLD_GLOBAL)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    L.rcn_create.restype = C.c_int
    L.rcn_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.rcn_destroy.restype = None
    L.rcn_destroy.argtypes = [vp]
    L.rcn_last_error.restype = C.c_char_p
    L.rcn_last_error.argtypes = [vp]
    L.rcn_version.restype = C.c_char_p
    L.rcn_version.argtypes = []
    L.rcn_set_stream.restype = C.c_int
    L.rcn_set_stream.argtypes = [vp, vp]
    L.rcn_synchronize.restype = C.c_int
    L.rcn_synchronize.argtypes = [vp]
    L.rcn_desc_upload.restype = C.c_int
    L.rcn_desc_upload.argtypes = [vp, i32, vp, i32, i32]
    L.rcn_desc_upload_device.restype = C.c_int
    L.rcn_desc_upload_device.argtypes = [vp, i32, vp, i32, i32]
    L.rcn_desc_upload_batch_device.restype = C.c_int
    L.rcn_desc_upload_batch_device.argtypes = [vp, i32, i32, vp, i32, i32]
    L.rcn_desc_upload_batch.restype = C.c_int
    L.rcn_desc_upload_batch.argtypes = [vp, i32, i32, vp, vp, i32]
    L.rcn_desc_remove.restype = C.c_int
    L.rcn_desc_remove.argtypes = [vp, i32]
    L.rcn_desc_sample_device.restype = C.c_int
    L.rcn_desc_sample_device.argtypes = [vp, vp, i64, i64, i64, i32, i32, vp, i32, i32, vp]
    L.rcn_desc_sample_errors.restype = C.c_int
    L.rcn_desc_sample_errors.argtypes = [vp, C.POINTER(i32)]
    L.rcn_desc_sample_batch_device.restype = C.c_int
    L.rcn_desc_sample_batch_device.argtypes = [vp, vp, i64, i64, i64, i64, i32, i32, vp, vp, i32, i32, i32, vp]
    L.rcn_kp_detect_device.restype = C.c_int
    L.rcn_kp_detect_device.argtypes = [vp, vp, i64, i64, i64, i64, i32, i32, i32, i32, C.c_double, i32, i32, i32, vp, vp, vp, vp, vp]
    L.rcn_kp_nms_device.restype = C.c_int
    L.rcn_kp_nms_device.argtypes = [vp, vp, i32, i32, i32, C.c_double, i32, i32, i32, vp, vp, vp, vp]
    L.rcn_sg_default_options.restype = None
    L.rcn_sg_default_options.argtypes = [C.POINTER(SgOptions)]
    sg_out = [vp, vp, vp, vp, vp, i64, vp, vp, vp]      # matches0/1, mscores0/1, table, stride, counts, logP, status
    L.rcn_sg_scores_device.restype = C.c_int
    L.rcn_sg_scores_device.argtypes = [vp, vp, i64, i64, i64, vp, i64, i64, i64, vp, vp, i32, i32, i32, i32, vp]
    L.rcn_sg_assign_device.restype = C.c_int
    L.rcn_sg_assign_device.argtypes = [vp, vp, i64, i64, i64, vp, vp, i32, i32, i32, C.POINTER(SgOptions)] + sg_out
    L.rcn_sg_match_device.restype = C.c_int
    L.rcn_sg_match_device.argtypes = [vp, vp, i64, i64, i64, vp, i64, i64, i64, vp, vp, i32, i32, i32, i32, C.POINTER(SgOptions)] + sg_out
    L.rcn_sg_set_chunk_bytes.restype = C.c_int
    L.rcn_sg_set_chunk_bytes.argtypes = [vp, i64]
    L.rcn_sg_net_create.restype = C.c_int
    L.rcn_sg_net_create.argtypes = [vp, vp, i32, vp, i64, C.c_double, C.POINTER(vp)]
    L.rcn_sg_net_destroy.restype = None
    L.rcn_sg_net_destroy.argtypes = [vp]
    L.rcn_sg_net_set_chunk_pairs.restype = C.c_int
    L.rcn_sg_net_set_chunk_pairs.argtypes = [vp, i32]
    sg_net_in = [vp, vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, i64, i64, i64, vp, vp, vp, vp, i32, i32, i32, i32]   # ctx, net, image 0, image 1, shapes, counts, B M N D
    L.rcn_sg_net_forward_device.restype = C.c_int
    L.rcn_sg_net_forward_device.argtypes = sg_net_in + [vp, vp]
    L.rcn_sg_net_match_device.restype = C.c_int
    L.rcn_sg_net_match_device.argtypes = sg_net_in + [C.POINTER(SgOptions)] + sg_out
    L.rcn_sp_net_create.restype = C.c_int
    L.rcn_sp_net_create.argtypes = [vp, vp, i64, C.POINTER(vp)]
    L.rcn_sp_net_destroy.restype = None
    L.rcn_sp_net_destroy.argtypes = [vp]
    L.rcn_sp_net_set_chunk_images.restype = C.c_int
    L.rcn_sp_net_set_chunk_images.argtypes = [vp, i32]
    sp_net_in = [vp, vp, vp, i32, i64, i64, i64, i32, i32, i32, i32]   # ctx, net, images, dtype, strides, n H W, flags
    L.rcn_sp_net_forward_device.restype = C.c_int
    L.rcn_sp_net_forward_device.argtypes = sp_net_in + [vp, vp]
    L.rcn_sp_net_detect_device.restype = C.c_int
    L.rcn_sp_net_detect_device.argtypes = sp_net_in + [i32, C.c_double, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.rcn_sift_default_options.restype = None
    L.rcn_sift_default_options.argtypes = [C.POINTER(SiftOptions)]
    L.rcn_sift_layout.restype = C.c_int
    L.rcn_sift_layout.argtypes = [i32, i32, C.POINTER(SiftOptions), C.POINTER(SiftLayout)]
    L.rcn_sift_set_chunk_images.restype = C.c_int
    L.rcn_sift_set_chunk_images.argtypes = [vp, i32]
    L.rcn_img_reshape_size.restype = C.c_int
    L.rcn_img_reshape_size.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_double)]
    L.rcn_img_resize_tables.restype = C.c_int
    L.rcn_img_resize_tables.argtypes = [i32, i32, i32, vp, vp, C.POINTER(i32)]
    L.rcn_img_default_options.restype = None
    L.rcn_img_default_options.argtypes = [C.POINTER(ImgOptions)]
    L.rcn_img_prepare_plan.restype = C.c_int
    L.rcn_img_prepare_plan.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.rcn_img_prepare_device.restype = C.c_int
    L.rcn_img_prepare_device.argtypes = [vp, vp, i64, i64, i32, i32, i32, i32, i32, i32, C.POINTER(ImgOptions), vp, vp]
    L.rcn_feat_colors_device.restype = C.c_int
    L.rcn_feat_colors_device.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, vp]
    L.rcn_landmark_colors_device.restype = C.c_int
    L.rcn_landmark_colors_device.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    L.rcn_cloud_vertices_device.restype = C.c_int
    L.rcn_cloud_vertices_device.argtypes = [vp, vp, vp, vp, i32, vp, i32, vp, C.POINTER(i64)]
    L.rcn_cloud_write_ply.restype = C.c_int
    L.rcn_cloud_write_ply.argtypes = [C.c_char_p, vp, i64, i32]
    sift_img = [vp, vp, i32, i64, i64, i64, i32, i32, i32, C.POINTER(SiftOptions)]     # ctx, images, dtype, strides, n H W, options
    sift_kp = [vp, vp, vp, vp, vp, vp, vp]                                              # xy, xy_int, size, angle, response, octave, counts
    L.rcn_sift_pyramid_device.restype = C.c_int
    L.rcn_sift_pyramid_device.argtypes = sift_img + [vp]
    L.rcn_sift_candidates_device.restype = C.c_int
    L.rcn_sift_candidates_device.argtypes = [vp, vp, i32, i32, i32, C.POINTER(SiftOptions), i32, vp, vp]
    L.rcn_sift_detect_device.restype = C.c_int
    L.rcn_sift_detect_device.argtypes = [vp, vp, i32, i32, i32, C.POINTER(SiftOptions), i32] + sift_kp
    L.rcn_sift_describe_device.restype = C.c_int
    L.rcn_sift_describe_device.argtypes = [vp, vp, i32, i32, i32, C.POINTER(SiftOptions), i32, vp, vp, vp, vp, vp, vp]
    L.rcn_sift_detect_and_compute_device.restype = C.c_int
    L.rcn_sift_detect_and_compute_device.argtypes = sift_img + [i32] + sift_kp + [vp]
    L.rcn_orb_default_options.restype = None
    L.rcn_orb_default_options.argtypes = [C.POINTER(OrbOptions)]
    L.rcn_orb_default_pattern.restype = C.POINTER(C.c_int8)
    L.rcn_orb_default_pattern.argtypes = []
    L.rcn_orb_layout.restype = C.c_int
    L.rcn_orb_layout.argtypes = [i32, i32, C.POINTER(OrbOptions), C.POINTER(OrbLayout)]
    L.rcn_orb_set_chunk_images.restype = C.c_int
    L.rcn_orb_set_chunk_images.argtypes = [vp, i32]
    orb_img = [vp, vp, i32, i64, i64, i64, i32, i32, i32, C.POINTER(OrbOptions)]       # ctx, images, dtype, strides, n H W, options
    orb_pyr = [vp, vp, i32, i32, i32, C.POINTER(OrbOptions)]                           # ctx, pyramids, n H W, options
    L.rcn_orb_pyramid_device.restype = C.c_int
    L.rcn_orb_pyramid_device.argtypes = orb_img + [vp]
    L.rcn_orb_fast_device.restype = C.c_int
    L.rcn_orb_fast_device.argtypes = orb_pyr + [vp]
    L.rcn_orb_detect_device.restype = C.c_int
    L.rcn_orb_detect_device.argtypes = orb_pyr + [i32] + sift_kp
    L.rcn_orb_describe_device.restype = C.c_int
    L.rcn_orb_describe_device.argtypes = orb_pyr + [i32, vp, vp, vp, vp, vp]
    L.rcn_orb_detect_and_compute_device.restype = C.c_int
    L.rcn_orb_detect_and_compute_device.argtypes = orb_img + [i32] + sift_kp + [vp, vp]
    L.rcn_bits_upload.restype = C.c_int
    L.rcn_bits_upload.argtypes = [vp, i32, vp, i32, i32]
    L.rcn_bits_upload_batch_device.restype = C.c_int
    L.rcn_bits_upload_batch_device.argtypes = [vp, i32, i32, vp, vp, i32, i32]
    L.rcn_bits_remove.restype = C.c_int
    L.rcn_bits_remove.argtypes = [vp, i32]
    L.rcn_bits_clear.restype = C.c_int
    L.rcn_bits_clear.argtypes = [vp]
    L.rcn_bits_count.restype = C.c_int
    L.rcn_bits_count.argtypes = [vp]
    L.rcn_match_pair_hamming.restype = C.c_int
    L.rcn_match_pair_hamming.argtypes = [vp, vp, i32, vp, i32, i32, f32, vp, C.POINTER(i32)]
    for fn in (L.rcn_match_grid_hamming, L.rcn_match_grid_hamming_device):
        fn.restype = C.c_int
        fn.argtypes = [vp, vp, i32, f32, vp, i64, vp]
    L.rcn_hamming_knn2_device.restype = C.c_int
    L.rcn_hamming_knn2_device.argtypes = [vp, vp, i32, vp, i64]
    L.rcn_guided_default_options.restype = C.c_int
    L.rcn_guided_default_options.argtypes = [C.POINTER(GuidedOptions)]
    for fn in (L.rcn_match_guided_device, L.rcn_match_guided):
        fn.restype = C.c_int
        fn.argtypes = [vp, vp, i32, vp, C.POINTER(GuidedOptions), vp, i64, vp, vp]
    L.rcn_match_pair_guided.restype = C.c_int
    L.rcn_match_pair_guided.argtypes = [vp, vp, i32, vp, vp, i32, vp, i32, vp, C.POINTER(GuidedOptions), vp, C.POINTER(i32)]
    L.rcn_guided_knn2_device.restype = C.c_int
    L.rcn_guided_knn2_device.argtypes = [vp, vp, i32, vp, f32, vp, vp, i64]
    L.rcn_match_table_filter_model_device.restype = C.c_int
    L.rcn_match_table_filter_model_device.argtypes = [vp, vp, i32, vp, i64, vp, vp, vp]
    L.rcn_match_grid_guided.restype = C.c_int
    L.rcn_match_grid_guided.argtypes = [vp, vp, i32, f32, C.POINTER(GuidedOptions), vp, i64, vp, vp]
    L.rcn_tracks_default_options.restype = None
    L.rcn_tracks_default_options.argtypes = [C.POINTER(TracksOptions)]
    L.rcn_tracks_layout.restype = C.c_int
    L.rcn_tracks_layout.argtypes = [vp, vp, vp, C.POINTER(i32)]
    for fn in (L.rcn_tracks_build_device, L.rcn_tracks_build):
        fn.restype = C.c_int
        fn.argtypes = [vp, C.POINTER(TracksOptions), i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rcn_tracks_last_phase_ms.restype = C.c_int
    L.rcn_tracks_last_phase_ms.argtypes = [vp, vp]
    L.rcn_retr_default_options.restype = None
    L.rcn_retr_default_options.argtypes = [C.POINTER(RetrOptions)]
    L.rcn_retr_codebook_train_device.restype = C.c_int
    L.rcn_retr_codebook_train_device.argtypes = [vp, vp, vp, i32, i32, i32, C.POINTER(RetrOptions), C.POINTER(vp)]
    L.rcn_retr_codebook_create.restype = C.c_int
    L.rcn_retr_codebook_create.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
    L.rcn_retr_codebook_read.restype = C.c_int
    L.rcn_retr_codebook_read.argtypes = [vp, vp, C.POINTER(i32), C.POINTER(i32)]
    L.rcn_retr_codebook_destroy.restype = None
    L.rcn_retr_codebook_destroy.argtypes = [vp]
    L.rcn_retr_assign_device.restype = C.c_int
    L.rcn_retr_assign_device.argtypes = [vp, vp, vp, i64, vp]
    L.rcn_retr_encode_device.restype = C.c_int
    L.rcn_retr_encode_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    L.rcn_retr_similarity_device.restype = C.c_int
    L.rcn_retr_similarity_device.argtypes = [vp, vp, i32, i32, i32, vp]
    L.rcn_retr_topk_device.restype = C.c_int
    L.rcn_retr_topk_device.argtypes = [vp, vp, i32, i32, vp]
    L.rcn_retr_pairs_device.restype = C.c_int
    L.rcn_retr_pairs_device.argtypes = [vp, vp, i32, i32, i32, vp, i64, vp]
    L.rcn_retr_image_pairs.restype = C.c_int
    L.rcn_retr_image_pairs.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i64, C.POINTER(i32)]
    L.rcn_desc_clear.restype = C.c_int
    L.rcn_desc_clear.argtypes = [vp]
    L.rcn_desc_count.restype = C.c_int
    L.rcn_desc_count.argtypes = [vp]
    L.rcn_match_pair.restype = C.c_int
    L.rcn_match_pair.argtypes = [vp, vp, i32, vp, i32, i32, f32, vp, C.POINTER(i32)]
    L.rcn_match_grid.restype = C.c_int
    L.rcn_match_grid.argtypes = [vp, vp, i32, f32, vp, i64, vp]
    L.rcn_match_grid_device.restype = C.c_int
    L.rcn_match_grid_device.argtypes = [vp, vp, i32, f32, vp, i64, vp]
    L.rcn_match_last_stats.restype = C.c_int
    L.rcn_match_last_stats.argtypes = [vp, C.POINTER(MatchStats)]
    L.rcn_match_profile.restype = C.c_int
    L.rcn_match_profile.argtypes = [vp, C.c_int]
    L.rcn_ba_default_options.restype = None
    L.rcn_ba_default_options.argtypes = [i32, C.POINTER(BaOptions)]
    L.rcn_ba_solve.restype = C.c_int
    L.rcn_ba_solve.argtypes = [vp, C.POINTER(BaProblem), C.POINTER(BaOptions), C.POINTER(BaSummary)]
    L.rcn_ba_solve_robust.restype = C.c_int
    L.rcn_ba_solve_robust.argtypes = [vp, C.POINTER(BaProblem), C.POINTER(BaOptions), C.POINTER(BaLoss), C.POINTER(BaSummary), C.POINTER(BaLossReport), vp]
    for fn in (L.rcn_landmark_validity, L.rcn_landmark_validity_device):
        fn.restype = C.c_int
        fn.argtypes = [vp, C.POINTER(LandmarkProblem), C.c_double, C.c_double, vp, vp, vp]
    L.rcn_fmat_filter.restype = C.c_int
    L.rcn_fmat_filter.argtypes = [vp, vp, vp, i32, vp, vp, vp]
    for fn in (L.rcn_fmat_filter_grid, L.rcn_fmat_filter_grid_device):
        fn.restype = C.c_int
        fn.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.rcn_coords_upload.restype = C.c_int
    L.rcn_coords_upload.argtypes = [vp, i32, vp, i32]
    L.rcn_coords_upload_batch.restype = C.c_int
    L.rcn_coords_upload_batch.argtypes = [vp, i32, i32, vp, vp]
    L.rcn_coords_clear.restype = C.c_int
    L.rcn_coords_clear.argtypes = [vp]
    L.rcn_match_table_filter_device.restype = C.c_int
    L.rcn_match_table_filter_device.argtypes = [vp, vp, i32, vp, C.c_int64, vp, vp]
    L.rcn_host_alloc.restype = C.c_int
    L.rcn_host_alloc.argtypes = [C.POINTER(vp), C.c_size_t]
    L.rcn_host_free.restype = None
    L.rcn_host_free.argtypes = [vp]
    L.rcn_match_compact_begin.restype = C.c_int
    L.rcn_match_compact_begin.argtypes = [vp, vp, i64, vp, i32, vp, vp, i64, C.POINTER(i64)]
    L.rcn_match_compact_wait.restype = C.c_int
    L.rcn_match_compact_wait.argtypes = [vp]
    L.rcn_shard_owned_images.restype = C.c_int
    L.rcn_shard_owned_images.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.rcn_shard_pair_count.restype = i64
    L.rcn_shard_pair_count.argtypes = [i32, i32, i32]
    L.rcn_shard_pairs.restype = C.c_int
    L.rcn_shard_pairs.argtypes = [i32, i32, i32, vp]
    L.rcn_shard_unique_id.restype = C.c_int
    L.rcn_shard_unique_id.argtypes = [vp]
    L.rcn_shard_create.restype = C.c_int
    L.rcn_shard_create.argtypes = [vp, i32, i32, vp, C.POINTER(vp)]
    L.rcn_shard_destroy.restype = None
    L.rcn_shard_destroy.argtypes = [vp]
    L.rcn_shard_ctx.restype = vp
    L.rcn_shard_ctx.argtypes = [vp]
    L.rcn_shard_reserve.restype = C.c_int
    L.rcn_shard_reserve.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    L.rcn_shard_exchange.restype = C.c_int
    L.rcn_shard_exchange.argtypes = [vp, vp, vp]
    L.rcn_shard_put_image.restype = C.c_int
    L.rcn_shard_put_image.argtypes = [vp, i32, vp, i32]
    L.rcn_shard_lists.restype = C.c_int
    L.rcn_shard_lists.argtypes = [vp, vp, vp, i64, C.POINTER(i64)]
    L.rcn_device_count.restype = C.c_int
    L.rcn_device_count.argtypes = []
    L.rcn_shard_match.restype = C.c_int
    L.rcn_shard_match.argtypes = [vp, f32, vp, i64, vp]
    L.rcn_shard_info.restype = C.c_int
    L.rcn_shard_info.argtypes = [vp, C.POINTER(ShardStats)]
    L.rcn_shard_filter.restype = C.c_int
    L.rcn_shard_filter.argtypes = [vp, vp]
    L.rcn_match_grid_filtered.restype = C.c_int
    L.rcn_match_grid_filtered.argtypes = [vp, vp, i32, f32, i32, vp, i64, vp, vp]
    L.rcn_shard_fail.restype = C.c_int
    L.rcn_shard_fail.argtypes = [vp, i32]
    L.rcn_shard_set_timeout.restype = C.c_int
    L.rcn_shard_set_timeout.argtypes = [vp, C.c_double]
    L.rcn_shard_gather_lists.restype = C.c_int
    L.rcn_shard_gather_lists.argtypes = [vp, i32, vp, i64, vp, vp, vp, i64, C.POINTER(i64)]
    L.rcn_shard_merge_lists.restype = C.c_int
    L.rcn_shard_merge_lists.argtypes = [i32, i32, vp, vp, vp, vp, i64, C.POINTER(i64)]
    L.rcn_shard_profile.restype = C.c_int
    L.rcn_shard_profile.argtypes = [vp, C.c_int]
    L.rcn_shard_profile_read.restype = C.c_int
    L.rcn_shard_profile_read.argtypes = [vp, C.POINTER(ShardTimes)]
    L.rcn_ba_solve_constant.restype = C.c_int
    L.rcn_ba_solve_constant.argtypes = [vp, C.POINTER(BaProblem), C.POINTER(BaOptions), C.POINTER(BaLoss), vp, C.POINTER(BaSummary), C.POINTER(BaLossReport), vp]
    L.rcn_ba_session_solve_local.restype = C.c_int
    L.rcn_ba_session_solve_local.argtypes = [vp, vp, i32, C.POINTER(BaOptions), C.POINTER(BaSummary), vp]
    L.rcn_ba_session_covisible.restype = C.c_int
    L.rcn_ba_session_covisible.argtypes = [vp, i32, i32, vp, C.POINTER(i32), vp]
    L.rcn_ba_session_local_seconds.restype = C.c_int
    L.rcn_ba_session_local_seconds.argtypes = [vp, vp]
    L.rcn_ba_session_create.restype = C.c_int
    L.rcn_ba_session_create.argtypes = [vp, C.POINTER(vp)]
    L.rcn_ba_session_destroy.restype = None
    L.rcn_ba_session_destroy.argtypes = [vp]
    L.rcn_ba_session_add_camera.restype = C.c_int
    L.rcn_ba_session_add_camera.argtypes = [vp, vp, vp, C.POINTER(i32)]
    L.rcn_ba_session_cameras.restype = C.c_int
    L.rcn_ba_session_cameras.argtypes = [vp, vp, vp, vp, vp]
    L.rcn_ba_session_add_points.restype = C.c_int
    L.rcn_ba_session_add_points.argtypes = [vp, i32, vp, C.POINTER(i32)]
    L.rcn_ba_session_add_observations.restype = C.c_int
    L.rcn_ba_session_add_observations.argtypes = [vp, i32, vp, vp, vp]
    L.rcn_ba_session_counts.restype = C.c_int
    L.rcn_ba_session_counts.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    L.rcn_ba_session_graph.restype = C.c_int
    L.rcn_ba_session_graph.argtypes = [vp, vp, vp, vp]
    L.rcn_ba_session_solve.restype = C.c_int
    L.rcn_ba_session_solve.argtypes = [vp, C.POINTER(BaOptions), C.POINTER(BaSummary)]
    L.rcn_ba_solve_tied.restype = C.c_int
    L.rcn_ba_solve_tied.argtypes = [vp, C.POINTER(BaProblem), C.POINTER(BaOptions), C.POINTER(BaLoss), vp, vp, C.POINTER(BaSummary), C.POINTER(BaLossReport), vp]
    L.rcn_ba_session_set_groups.restype = C.c_int
    L.rcn_ba_session_set_groups.argtypes = [vp, vp, i32]
    L.rcn_ba_session_set_loss.restype = C.c_int
    L.rcn_ba_session_set_loss.argtypes = [vp, C.POINTER(BaLoss)]
    L.rcn_ba_session_loss_report.restype = C.c_int
    L.rcn_ba_session_loss_report.argtypes = [vp, C.POINTER(BaLossReport), vp]
    L.rcn_ba_session_read_points.restype = C.c_int
    L.rcn_ba_session_read_points.argtypes = [vp, vp]
    L.rcn_ba_session_points_device.restype = vp
    L.rcn_ba_session_points_device.argtypes = [vp]
    L.rcn_ba_session_validity.restype = C.c_int
    L.rcn_ba_session_validity.argtypes = [vp, vp, C.c_double, C.c_double, vp, C.POINTER(i32), C.POINTER(i32)]
    L.rcn_ba_session_remove_outliers.restype = C.c_int
    L.rcn_ba_session_remove_outliers.argtypes = [vp, vp, C.POINTER(i32)]
    L.rcn_ba_session_triangulate.restype = C.c_int
    L.rcn_ba_session_triangulate.argtypes = [vp, vp, i32, vp, vp, vp, C.c_double, C.c_double, vp, C.POINTER(i32), C.POINTER(i32)]
    L.rcn_triangulate.restype = C.c_int
    L.rcn_triangulate.argtypes = [vp, C.POINTER(TriangulationProblem), C.c_double, C.c_double, vp, vp, vp]
    L.rcn_triangulate_device.restype = C.c_int
    L.rcn_triangulate_device.argtypes = [vp, C.POINTER(TriangulationProblem), C.c_double, C.c_double, vp, vp, vp, i32, vp]
    L.rcn_match_lists_upload.restype = C.c_int
    L.rcn_match_lists_upload.argtypes = [vp, i32, vp, vp, vp, i32]
    L.rcn_match_lists_clear.restype = C.c_int
    L.rcn_match_lists_clear.argtypes = [vp]
    L.rcn_corr_set_workspace_bytes.restype = C.c_int
    L.rcn_corr_set_workspace_bytes.argtypes = [vp, i64]
    L.rcn_corr_2d3d.restype = C.c_int
    L.rcn_corr_2d3d.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, i64, C.POINTER(i64), vp, vp]
    L.rcn_corr_2d3d_device.restype = C.c_int
    L.rcn_corr_2d3d_device.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp]
    L.rcn_landmark_attach.restype = C.c_int
    L.rcn_landmark_attach.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp, vp, C.c_double, vp, C.POINTER(i32)]
    L.rcn_ba_session_attach.restype = C.c_int
    L.rcn_ba_session_attach.argtypes = [vp, vp, i32, i32, vp, vp, vp, C.c_double, vp, C.POINTER(i32)]
    L.rcn_landmark_ids_reset.restype = C.c_int
    L.rcn_landmark_ids_reset.argtypes = [vp]
    L.rcn_landmark_ids_set.restype = C.c_int
    L.rcn_landmark_ids_set.argtypes = [vp, i32, vp, vp, vp]
    L.rcn_landmark_ids_read.restype = C.c_int
    L.rcn_landmark_ids_read.argtypes = [vp, i32, vp, i32]
    L.rcn_new_view_tracks_device.restype = C.c_int
    L.rcn_new_view_tracks_device.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.rcn_new_view_triangulate_device.restype = C.c_int
    L.rcn_new_view_triangulate_device.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, vp, C.c_double, C.c_double, i32, i32,
                                                  vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    L.rcn_ba_session_grow_view.restype = C.c_int
    L.rcn_ba_session_grow_view.argtypes = [vp, vp, i32, i32, i32, vp, vp, C.c_double, C.c_double, C.POINTER(i32), vp, vp,
                                           C.POINTER(i32), C.POINTER(i32)]
    L.rcn_pnp_default_options.restype = None
    L.rcn_pnp_default_options.argtypes = [C.POINTER(PnpOptions)]
    L.rcn_pnp_ransac.restype = C.c_int
    L.rcn_pnp_ransac.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, C.POINTER(PnpOptions), vp, vp, vp, vp, vp]
    L.rcn_pnp_ransac_device.restype = C.c_int
    L.rcn_pnp_ransac_device.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp, C.POINTER(PnpOptions), vp, vp, vp, vp, vp]
    L.rcn_ba_session_pnp.restype = C.c_int
    L.rcn_ba_session_pnp.argtypes = [vp, i32, vp, vp, vp, C.POINTER(PnpOptions), vp, vp, C.POINTER(i32)]
    L.rcn_twoview_default_options.restype = None
    L.rcn_twoview_default_options.argtypes = [C.POINTER(TwoViewOptions)]
    L.rcn_twoview_init.restype = C.c_int
    L.rcn_twoview_init.argtypes = [vp, i32, vp, vp, vp, vp, vp, C.POINTER(TwoViewOptions), vp, vp, vp, vp, vp, vp]
    L.rcn_twoview_init_device.restype = C.c_int
    L.rcn_twoview_init_device.argtypes = [vp, i32, vp, vp, vp, C.POINTER(TwoViewOptions), i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rcn_homography_default_options.restype = None
    L.rcn_homography_default_options.argtypes = [C.POINTER(HomographyOptions)]
    L.rcn_homography_ransac.restype = C.c_int
    L.rcn_homography_ransac.argtypes = [vp, i32, vp, vp, vp, C.POINTER(HomographyOptions), vp, vp, vp, vp]
    L.rcn_homography_ransac_device.restype = C.c_int
    L.rcn_homography_ransac_device.argtypes = [vp, i32, vp, C.POINTER(HomographyOptions), i64, vp, vp, vp, vp, vp, vp]
    L.rcn_twoview_geometry_default_options.restype = None
    L.rcn_twoview_geometry_default_options.argtypes = [C.POINTER(TwoViewGeometryOptions)]
    L.rcn_twoview_geometry.restype = C.c_int
    L.rcn_twoview_geometry.argtypes = [vp, i32, vp, vp, vp, vp, vp, C.POINTER(TwoViewOptions), C.POINTER(HomographyOptions),
                                       C.POINTER(TwoViewGeometryOptions)] + [vp] * 13
    L.rcn_twoview_geometry_device.restype = C.c_int
    L.rcn_twoview_geometry_device.argtypes = [vp, i32, vp, vp, vp, C.POINTER(TwoViewOptions), C.POINTER(HomographyOptions),
                                              C.POINTER(TwoViewGeometryOptions), i64] + [vp] * 15
    L.rcn_pose34_to_pose6.restype = C.c_int
    L.rcn_pose34_to_pose6.argtypes = [vp, vp]
    L.rcn_ba_session_init_pair.restype = C.c_int
    L.rcn_ba_session_init_pair.argtypes = [vp, i32, vp, vp, vp, vp, C.POINTER(TwoViewOptions), C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, vp,
                                           C.POINTER(i32)]
    L.rcn_mvs_default_options.restype = None
    L.rcn_mvs_default_options.argtypes = [C.POINTER(MvsOptions)]
    L.rcn_mvs_layout.restype = C.c_int
    L.rcn_mvs_layout.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(MvsSizes)]
    L.rcn_mvs_inv_depths.restype = C.c_int
    L.rcn_mvs_inv_depths.argtypes = [C.c_double, C.c_double, i32, vp]
    L.rcn_mvs_homographies.restype = C.c_int
    L.rcn_mvs_homographies.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp]
    L.rcn_img_undistort_device.restype = C.c_int
    L.rcn_img_undistort_device.argtypes = [vp, vp, i64, i64, i32, i32, i32, i32, vp, vp]
    L.rcn_mvs_sweep_device.restype = C.c_int
    L.rcn_mvs_sweep_device.argtypes = [vp, vp, i64, i64, i32, i32, i32, vp, i32, i32, vp, vp, i32, C.POINTER(MvsOptions), vp, vp, vp]
    L.rcn_mvs_consistency_device.restype = C.c_int
    L.rcn_mvs_consistency_device.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, i32, vp, vp, C.POINTER(MvsOptions), vp, vp]
    L.rcn_mvs_fuse_device.restype = C.c_int
    L.rcn_mvs_fuse_device.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, i32, i32, vp, vp, C.POINTER(MvsOptions), i64, vp, vp]
    L.rcn_ba_session_mvs_views.restype = C.c_int
    L.rcn_ba_session_mvs_views.argtypes = [vp, vp, i32, vp, vp, vp]
    L.rcn_store_save.restype = C.c_int
    L.rcn_store_save.argtypes = [C.c_char_p, C.POINTER(StoreContents)]
    L.rcn_store_open.restype = C.c_int
    L.rcn_store_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.rcn_store_contents_of.restype = C.c_int
    L.rcn_store_contents_of.argtypes = [vp, C.POINTER(StoreContents)]
    L.rcn_store_close.restype = None
    L.rcn_store_close.argtypes = [vp]
    L.rcn_store_upload.restype = C.c_int
    L.rcn_store_upload.argtypes = [vp, vp]
    _LIB = L
    return L


class Context:
    """One rcn_ctx (one GPU)."""

    def __init__(self, device=0):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.rcn_create(int(device), C.byref(h))
        if rc != RCN_OK:
            raise RcnError(rc, "rcn_create(device=%d): no usable gfx950 device" % device)
        self.h = h
        self.device = device

    def check(self, rc):
        if rc != RCN_OK:
            raise RcnError(rc, self.lib.rcn_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.rcn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
