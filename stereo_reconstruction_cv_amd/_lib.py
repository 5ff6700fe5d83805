"""ctypes binding of include/sgm_hip.h (the C ABI of the HIP library).

The product path has no CPU fallback: if the shared library is missing, or there is no GPU,
every compute entry point raises.  Nothing in this package imports the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SGM_HIP_LIB: developer override (A/B runs of experimental builds); the product path is the in-tree library
LIB_PATH = os.environ.get("SGM_HIP_LIB") or os.path.join(_HERE, "csrc", "libsgm_hip.so")

SGM_OK = 0
SGM_TAP_COST, SGM_TAP_AGGR, SGM_TAP_DISP_RAW, SGM_TAP_DISP_MEDIAN = 0, 1, 2, 3
SGM_TAP_CONF_RAW, SGM_TAP_CONF = 4, 5    # uint8 (H, W) match confidence: the uniqueness margin, and the same masked by the final map
SGM_TAP_RIGHT_RAW, SGM_TAP_RIGHT = 6, 7  # int16 (H, W) right-view disparity: after the right-to-left check, and after median + speckle filter
SGM_OPT_KEEP_AGGR, SGM_OPT_PROFILE, SGM_OPT_SCHEDULE, SGM_OPT_SWEEP_ROWS, SGM_OPT_PREPASS_ROWS, SGM_OPT_CHAIN_WGS, SGM_OPT_GROUP_MAX = 0, 1, 2, 3, 5, 6, 7
SGM_OPT_CHANNELS = 8    # 1 (default) or 3: interleaved 8-bit channels per image pixel
SGM_OPT_CONFIDENCE = 10  # 1: every compute also produces the confidence maps (SGM_TAP_CONF_RAW, SGM_TAP_CONF)
SGM_OPT_RIGHT_VIEW = 11  # 1: every compute also produces the right-view map (SGM_TAP_RIGHT_RAW, SGM_TAP_RIGHT)
SGM_OPT_COST = 12        # the matching cost of every compute on the engine: SGM_COST_BT (default) or SGM_COST_CENSUS
SGM_COST_BT, SGM_COST_CENSUS = 0, 1
SGM_OPT_DEBUG = 4    # csrc/sgm_debug.h: A/B switches for tools/ and tests/, not part of the public interface
SGM_OPT_POISON = 9   # csrc/sgm_debug.h: fill every device buffer with a byte (0..255) and arm the same for new ones; -1 disarms (tests only)
SGM_DBG_VOXEL_TIGHT_TABLE, SGM_DBG_VOXEL_OTHER_REDUCTION = 1 << 22, 1 << 23   # csrc/sgm_debug.h: the two A/B bits of sgm_voxel_downsample
SGM_DBG_RADIUS_TIGHT_TABLE, SGM_DBG_RADIUS_SOURCE_ORDER = 1 << 24, 1 << 25   # csrc/sgm_debug.h: the two A/B bits of sgm_radius_outlier
SGM_DBG_STAT_WIDE_LIST = 1 << 26   # csrc/sgm_debug.h: the A/B bit of sgm_statistical_outlier (the 64-word list at every nb_neighbors)
SGM_DBG_COV_SEPARATE_SOLVE, SGM_DBG_COV_SELECT_ACCUM = 1 << 27, 1 << 28   # csrc/sgm_debug.h: the two A/B bits of sgm_covariance_normals
SGM_DBG_DBSCAN_GATHER_CORE = 1 << 29   # csrc/sgm_debug.h: the A/B bit of sgm_cluster_dbscan (the core bit gathered by source index)
SGM_DBG_PLANE_OTHER_COUNT = 1 << 30   # csrc/sgm_debug.h: the A/B bit of sgm_segment_plane (step 5 by the form that is not the default)
SGM_MAX_STAGES = 32

# every symbol include/sgm_hip.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "sgm_abi_version", "sgm_device_count", "sgm_last_error", "sgm_create", "sgm_destroy",
    "sgm_set_option", "sgm_geometry", "sgm_compute", "sgm_compute_batch", "sgm_disp_to_float",
    "sgm_reproject", "sgm_valid_mask", "sgm_get_tap", "sgm_get_headroom", "sgm_median3x3", "sgm_filter_speckles", "sgm_compact_points",
    "sgm_compact_points_device", "sgm_compact_points_device_async", "sgm_compute_device", "sgm_check", "sgm_trim",
    "sgm_disp_to_float_device", "sgm_reproject_device", "sgm_valid_mask_device",
    "sgm_pipeline_device", "sgm_pipeline_batch_device", "sgm_synchronize", "sgm_get_stage_times", "sgm_algorithmic_bytes",
    "sgm_init_undistort_rectify_map", "sgm_init_undistort_rectify_map_device",
    "sgm_remap_linear_u8", "sgm_remap_linear_u8_device",
)
# include/sgm_hip_confidence.h (included by sgm_hip.h): the entry point added with SGM_OPT_CONFIDENCE
CONFIDENCE_EXPORTS = ("sgm_bind_confidence_device",)
# include/sgm_hip_right.h (likewise): the entry point added with SGM_OPT_RIGHT_VIEW
RIGHT_EXPORTS = ("sgm_bind_right_device",)
# include/sgm_hip_wls.h (likewise): the edge-aware disparity post-filter
WLS_EXPORTS = ("sgm_wls_weights", "sgm_wls_filter", "sgm_wls_filter_device")
# include/sgm_hip_wls_batch.h (likewise): the filter over N maps of one shape per call
WLS_BATCH_EXPORTS = ("sgm_wls_filter_batch", "sgm_wls_filter_batch_device")
# include/sgm_hip_lrc.h (likewise): the left-right consistency confidence from a left-view and a right-view map
LRC_EXPORTS = ("sgm_lrc_confidence", "sgm_lrc_confidence_device", "sgm_lrc_confidence_batch_device")
# include/sgm_hip_voxel.h (likewise): voxel-grid downsampling of the point cloud
VOXEL_EXPORTS = ("sgm_voxel_downsample", "sgm_voxel_downsample_device")
# include/sgm_hip_mesh.h (likewise): the triangle mesh from the organised cloud
MESH_EXPORTS = ("sgm_mesh_grid", "sgm_mesh_grid_device")
# include/sgm_hip_normals.h (likewise): the vertex normals of that mesh and the normal image of the organised cloud
NORMALS_EXPORTS = ("sgm_normals_grid", "sgm_normals_grid_device", "sgm_mesh_grid_normals", "sgm_mesh_grid_normals_device")
# include/sgm_hip_radius.h (likewise): radius outlier removal for the point cloud
RADIUS_EXPORTS = ("sgm_radius_outlier", "sgm_radius_outlier_device")
# include/sgm_hip_statistical.h (likewise): statistical outlier removal for the point cloud
STATISTICAL_EXPORTS = ("sgm_statistical_outlier", "sgm_statistical_outlier_device")
# include/sgm_hip_covariance.h (likewise): covariance normals for a point list
COVARIANCE_EXPORTS = ("sgm_covariance_normals", "sgm_covariance_normals_device")
# the stage record of one sgm_covariance_normals call with SGM_OPT_PROFILE (cov_solve only with SGM_DBG_COV_SEPARATE_SOLVE)
COVARIANCE_STAGES = ("cov_count", "cov_clear", "cov_insert", "cov_starts", "cov_sort", "cov_query", "cov_solve")
# include/sgm_hip_dbscan.h (likewise): density clustering of the point cloud
DBSCAN_EXPORTS = ("sgm_cluster_dbscan", "sgm_cluster_dbscan_device")
# the stage record of one sgm_cluster_dbscan call with SGM_OPT_PROFILE
DBSCAN_STAGES = ("dbscan_count", "dbscan_clear", "dbscan_insert", "dbscan_starts", "dbscan_sort", "dbscan_core", "dbscan_link",
                 "dbscan_number", "dbscan_label")
# include/sgm_hip_plane.h (likewise): plane segmentation of the point cloud
PLANE_EXPORTS = ("sgm_segment_plane", "sgm_segment_plane_device", "sgm_plane_inliers", "sgm_plane_inliers_device")
# the stage record of one sgm_segment_plane call with SGM_OPT_PROFILE (plane_moments and plane_solve only with refine = 1;
# sgm_plane_inliers has the last two)
PLANE_STAGES = ("plane_valid", "plane_sample", "plane_count", "plane_best", "plane_moments", "plane_solve", "plane_classify",
                "plane_compact")
# include/sgm_hip_icp.h (likewise): rigid registration of two point clouds
ICP_EXPORTS = ("sgm_register_icp", "sgm_register_icp_device", "sgm_evaluate_registration", "sgm_evaluate_registration_device",
               "sgm_transform_points", "sgm_transform_points_device", "sgm_icp_solve")
# the stage record of one sgm_register_icp call with SGM_OPT_PROFILE: the target's grid, then the last evaluation
ICP_STAGES = ("icp_count", "icp_clear", "icp_insert", "icp_starts", "icp_sort", "icp_correspond", "icp_terms", "icp_reduce")
# include/sgm_hip_tsdf.h (likewise): the truncated signed distance volume
TSDF_EXPORTS = ("sgm_tsdf_integrate", "sgm_tsdf_integrate_device", "sgm_tsdf_extract_points", "sgm_tsdf_extract_points_device")
# the stage records with SGM_OPT_PROFILE: tsdf_integrate of an integration; the other three of an extraction (tsdf_emit unless it only counts)
TSDF_STAGES = ("tsdf_integrate", "tsdf_count", "tsdf_scan", "tsdf_emit")


class SgmParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff",
        "preFilterCap", "uniquenessRatio", "speckleWindowSize", "speckleRange", "mode")]


class SgmStageTimes(C.Structure):
    _fields_ = [("n", C.c_int32), ("name", C.c_char_p * SGM_MAX_STAGES),
                ("ms", C.c_float * SGM_MAX_STAGES), ("launches", C.c_int32 * SGM_MAX_STAGES)]


class SgmDebugPlan(C.Structure):
    """csrc/sgm_debug.h: sgm_debug_plan_t (test scaffolding, not part of the public interface)"""
    _fields_ = [(n, C.c_int32) for n in (
        "W1", "minX1", "NP", "partial", "byte_cost", "pix_px", "GWc", "RBb", "vsum_ring", "rows4", "GWs", "chain", "R", "nbands",
        "fused_prepass", "prepass_g", "pre_nch", "pre_rows", "overlap", "fused_wta", "nvol", "path_w_main", "speckle",
        "chain_window")]


class LibraryMissing(RuntimeError):
    pass


ABI_VERSION = 4   # include/sgm_hip.h: SGM_ABI_VERSION this binding was written against


_lib = None


def load():
    """Load libsgm_hip.so; raises LibraryMissing with build instructions when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C stereo_reconstruction_cv_amd/csrc` (there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    L.sgm_abi_version.restype = C.c_int
    if L.sgm_abi_version() != ABI_VERSION:      # a stale build: say so instead of an AttributeError at bind time
        raise LibraryMissing(
            f"{LIB_PATH} has ABI version {L.sgm_abi_version()}, this package needs {ABI_VERSION}: rebuild it "
            "(`make -C stereo_reconstruction_cv_amd/csrc`)")
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    pp = C.POINTER(SgmParams)
    L.sgm_abi_version.restype = i32
    L.sgm_device_count.restype = i32
    L.sgm_last_error.restype = C.c_char_p
    L.sgm_create.argtypes = [pp, i32, vp, C.POINTER(vp)]
    L.sgm_destroy.argtypes = [vp]
    L.sgm_destroy.restype = None
    L.sgm_set_option.argtypes = [vp, i32, i32]
    L.sgm_geometry.argtypes = [pp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.sgm_compute.argtypes = [vp, vp, vp, i32, i32, i64, vp]
    L.sgm_compute_batch.argtypes = [vp, i32, vp, vp, i32, i32, vp, vp, vp]
    L.sgm_disp_to_float.argtypes = [vp, vp, i64, vp]
    L.sgm_reproject.argtypes = [vp, vp, i32, i32, vp, i32, vp]
    L.sgm_valid_mask.argtypes = [vp, vp, vp, i64, vp]
    L.sgm_get_tap.argtypes = [vp, i32, vp, i64]
    L.sgm_get_headroom.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.sgm_median3x3.argtypes = [vp, vp, i32, i32, vp]
    L.sgm_filter_speckles.argtypes = [vp, vp, i32, i32, i32, i32, i32]
    L.sgm_compact_points.argtypes = [vp, vp, vp, vp, i64, vp, vp, C.POINTER(i64)]
    L.sgm_compact_points_device.argtypes = [vp, vp, vp, vp, i64, vp, vp, C.POINTER(i64)]
    L.sgm_compact_points_device_async.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp]
    L.sgm_check.argtypes = [vp]
    L.sgm_trim.argtypes = [vp]
    L.sgm_compute_device.argtypes = [vp, vp, vp, i32, i32, i64, vp]
    L.sgm_disp_to_float_device.argtypes = [vp, vp, i64, vp]
    L.sgm_reproject_device.argtypes = [vp, vp, i32, i32, vp, i32, vp]
    L.sgm_valid_mask_device.argtypes = [vp, vp, vp, i64, vp]
    L.sgm_pipeline_device.argtypes = [vp, vp, vp, i32, i32, i64, vp, vp, vp, vp]
    L.sgm_pipeline_batch_device.argtypes = [vp, i32, vp, vp, i32, i32, i64, vp, vp, vp, vp]
    L.sgm_bind_confidence_device.argtypes = [vp, i32, vp]
    L.sgm_bind_right_device.argtypes = [vp, i32, vp]
    L.sgm_wls_weights.argtypes = [C.c_double, vp]
    L.sgm_wls_filter.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, C.c_double, vp, vp, vp]
    L.sgm_wls_filter_device.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, C.c_double, vp, vp, vp]
    L.sgm_wls_filter_batch.argtypes = [vp, i32, vp, vp, i32, vp, i32, i32, i32, C.c_double, vp, vp, vp]
    L.sgm_wls_filter_batch_device.argtypes = [vp, i32, vp, vp, i32, vp, i32, i32, i32, C.c_double, vp, vp, vp]
    L.sgm_lrc_confidence.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]
    L.sgm_lrc_confidence_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]
    L.sgm_lrc_confidence_batch_device.argtypes = [vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]
    L.sgm_voxel_downsample.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_float, vp, i32, vp, vp, vp, vp, vp]
    L.sgm_voxel_downsample_device.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_float, vp, i32, vp, vp, vp, vp, vp]
    L.sgm_mesh_grid.argtypes = [vp, vp, vp, vp, i32, i32, C.c_float, vp, vp, vp, vp, vp]
    L.sgm_mesh_grid_device.argtypes = [vp, vp, vp, vp, i32, i32, C.c_float, vp, vp, vp, vp, vp]
    L.sgm_normals_grid.argtypes = [vp, vp, vp, i32, i32, C.c_float, i32, vp]
    L.sgm_normals_grid_device.argtypes = [vp, vp, vp, i32, i32, C.c_float, i32, vp]
    L.sgm_mesh_grid_normals.argtypes = [vp, vp, vp, vp, i32, i32, C.c_float, i32, vp, vp, vp, vp, vp, vp]
    L.sgm_mesh_grid_normals_device.argtypes = [vp, vp, vp, vp, i32, i32, C.c_float, i32, vp, vp, vp, vp, vp, vp]
    L.sgm_radius_outlier.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_float, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.sgm_radius_outlier_device.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_float, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.sgm_statistical_outlier.argtypes = [vp, vp, vp, vp, C.c_int64, i32, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp, vp, vp]
    L.sgm_statistical_outlier_device.argtypes = [vp, vp, vp, vp, C.c_int64, i32, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp, vp, vp]
    L.sgm_covariance_normals.argtypes = [vp, vp, vp, C.c_int64, C.c_float, i32, vp, vp, i32, vp, vp, vp, vp]
    L.sgm_covariance_normals_device.argtypes = [vp, vp, vp, C.c_int64, C.c_float, i32, vp, vp, i32, vp, vp, vp, vp]
    L.sgm_cluster_dbscan.argtypes = [vp, vp, vp, C.c_int64, C.c_float, i32, vp, vp, vp, vp, vp, vp]
    L.sgm_cluster_dbscan_device.argtypes = [vp, vp, vp, C.c_int64, C.c_float, i32, vp, vp, vp, vp, vp, vp]
    L.sgm_segment_plane.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_float, i32, C.c_uint32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.sgm_segment_plane_device.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_float, i32, C.c_uint32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.sgm_plane_inliers.argtypes = [vp, vp, vp, vp, C.c_int64, vp, C.c_float, i32, vp, vp, vp, vp, vp, vp, vp]
    L.sgm_plane_inliers_device.argtypes = [vp, vp, vp, vp, C.c_int64, vp, C.c_float, i32, vp, vp, vp, vp, vp, vp, vp]
    f64, dp = C.c_double, C.POINTER(C.c_double)
    L.sgm_register_icp.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_float, vp, vp, i32, i32, f64, f64, vp, dp, dp, vp, vp, vp, vp]
    L.sgm_register_icp_device.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_float, vp, vp, i32, i32, f64, f64, vp, dp, dp, vp, vp, vp, vp]
    L.sgm_evaluate_registration.argtypes = [vp, vp, vp, C.c_int64, vp, vp, C.c_int64, C.c_float, vp, vp, dp, dp, vp, vp, vp]
    L.sgm_evaluate_registration_device.argtypes = [vp, vp, vp, C.c_int64, vp, vp, C.c_int64, C.c_float, vp, vp, dp, dp, vp, vp, vp]
    L.sgm_transform_points.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp]
    L.sgm_transform_points_device.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp]
    L.sgm_icp_solve.argtypes = [vp, i32, vp, vp, C.POINTER(i32)]
    L.sgm_tsdf_integrate.argtypes = [vp, vp, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, i32, vp, C.c_float, vp]
    L.sgm_tsdf_integrate_device.argtypes = [vp, vp, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, i32, vp, C.c_float, vp]
    L.sgm_tsdf_extract_points.argtypes = [vp, vp, C.c_float, vp, vp, vp, vp, i32, i64, vp, vp, C.POINTER(i64)]
    L.sgm_tsdf_extract_points_device.argtypes = [vp, vp, C.c_float, vp, vp, vp, vp, i32, i64, vp, vp, C.POINTER(i64)]
    L.sgm_synchronize.argtypes = [vp]
    L.sgm_get_stage_times.argtypes = [vp, C.POINTER(SgmStageTimes)]
    L.sgm_algorithmic_bytes.argtypes = [pp, i32, i32, i32]
    L.sgm_algorithmic_bytes.restype = i64
    L.sgm_init_undistort_rectify_map.argtypes = [vp, vp, vp, i32, vp, vp, i32, i32, i32, vp, vp]
    L.sgm_init_undistort_rectify_map_device.argtypes = [vp, vp, vp, i32, vp, vp, i32, i32, i32, vp, vp]
    L.sgm_remap_linear_u8.argtypes = [vp, vp, i32, i32, i64, i32, vp, vp, i32, i32, vp]
    L.sgm_remap_linear_u8_device.argtypes = [vp, vp, i32, i32, i64, i32, vp, vp, i32, i32, vp, i64]
    # csrc/sgm_debug.h, outside EXPORTS: the plan readout for tests
    L.sgm_debug_plan.argtypes = [pp, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(SgmDebugPlan)]
    L.sgm_debug_plan.restype = i32
    L.sgm_debug_plan_opts.argtypes = [pp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(SgmDebugPlan)]
    L.sgm_debug_plan_opts.restype = i32
    L.sgm_debug_plan_cost.argtypes = [pp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(SgmDebugPlan)]
    L.sgm_debug_plan_cost.restype = i32
    # ... and the readouts of the split winner-take-all
    L.sgm_debug_uniq_threshold.argtypes = [i32, i32]
    L.sgm_debug_uniq_threshold.restype = i32
    L.sgm_debug_wta_split.argtypes = [pp, i32, i32, i32, i32, i32, i32, i32, i32]
    L.sgm_debug_wta_split.restype = i32
    L.sgm_debug_wta_raw_bytes.argtypes = [vp]
    L.sgm_debug_wta_raw_bytes.restype = C.c_longlong
    L.sgm_debug_wta_select_n.argtypes = [i32, i32, vp, i32, vp]
    L.sgm_debug_wta_select_n.restype = i32
    for name in EXPORTS + CONFIDENCE_EXPORTS + RIGHT_EXPORTS + WLS_EXPORTS + WLS_BATCH_EXPORTS + LRC_EXPORTS + VOXEL_EXPORTS + MESH_EXPORTS + NORMALS_EXPORTS + RADIUS_EXPORTS + STATISTICAL_EXPORTS + COVARIANCE_EXPORTS + DBSCAN_EXPORTS + PLANE_EXPORTS + ICP_EXPORTS + TSDF_EXPORTS:
        fn = getattr(L, name)
        if fn.restype is C.c_int and name not in ("sgm_abi_version", "sgm_device_count"):
            fn.restype = i32
    _lib = L
    return L


def last_error() -> str:
    return (load().sgm_last_error() or b"").decode("utf-8", "replace")


def debug_plan(params: dict, H: int, W: int, channels: int = 1, schedule: int = 1, sweep_rows: int = 0, prepass_rows: int = 0,
               debug: int = 0, frames: int = 1, confidence: int = 0, right_view: int = 0, cost: int = SGM_COST_BT) -> dict:
    """The schedule one compute of an H x W frame takes with these arguments and options (csrc/sgm_debug.h: sgm_debug_plan),
    as a dict of the fields of sgm_debug_plan_t.  Needs no GPU.  For tests: which plan a case takes is read, not assumed.
    confidence / right_view: SGM_OPT_CONFIDENCE / SGM_OPT_RIGHT_VIEW of the engine (the sibling readout sgm_debug_plan_opts);
    cost: its SGM_OPT_COST (sgm_debug_plan_cost)."""
    out = SgmDebugPlan()
    if cost != SGM_COST_BT:
        rc = load().sgm_debug_plan_cost(C.byref(SgmParams(**params)), H, W, channels, schedule, sweep_rows, prepass_rows, debug,
                                        frames, confidence, right_view, cost, C.byref(out))
    elif confidence or right_view:
        rc = load().sgm_debug_plan_opts(C.byref(SgmParams(**params)), H, W, channels, schedule, sweep_rows, prepass_rows, debug,
                                        frames, confidence, right_view, C.byref(out))
    else:
        rc = load().sgm_debug_plan(C.byref(SgmParams(**params)), H, W, channels, schedule, sweep_rows, prepass_rows, debug, frames,
                                   C.byref(out))
    if rc != SGM_OK:
        raise ValueError(f"sgm_debug_plan failed ({rc}): {last_error()}")
    return {n: getattr(out, n) for n, _ in SgmDebugPlan._fields_}


def debug_wta_split(params: dict, H: int, W: int, schedule: int = 2, sweep_rows: int = 0, debug: int = 0, confidence: int = 0,
                    right_view: int = 0, keep_aggr: int = 0) -> bool:
    """Whether one compute of an H x W frame with these options takes the split winner-take-all (csrc/sgm_debug.h:
    sgm_debug_wta_split; Plan::wta_split is not part of sgm_debug_plan_t).  Needs no GPU."""
    rc = load().sgm_debug_wta_split(C.byref(SgmParams(**params)), H, W, schedule, sweep_rows, debug, confidence, right_view, keep_aggr)
    if rc < 0:
        raise ValueError(f"sgm_debug_wta_split failed ({rc}): {last_error()}")
    return bool(rc)
