"""MI355X-native dense stereo disparity engine: drop-in for the reference's
cv2.StereoSGBM_create(...).compute() / cv2.reprojectImageTo3D() path (main.ipynb:655-670, 697).

    import stereo_reconstruction_cv_amd as cv2   # for this path only
"""
from .stereo import (CV_32F, STEREO_COST_BT, STEREO_COST_CENSUS, STEREO_SGBM_MODE_HH, STEREO_SGBM_MODE_HH4, STEREO_SGBM_MODE_SGBM,
                     STEREO_SGBM_MODE_SGBM_3WAY, Engine, StereoSGBM, StereoSGBM_create, clear_engine_cache, error,
                     get_device, get_engine, reprojectImageTo3D, set_device, initUndistortRectifyMap, remap, CV_32FC1,
                     INTER_LINEAR, BORDER_CONSTANT, DisparityWLSFilter, createDisparityWLSFilter, wls_weights,
                     lrcConfidence)
from .pipeline import compute_disparity_map, reconstruct_3D, rectify_pair, run_disparity, valid_point_mask
from .pointcloud import (cluster_dbscan, largest_clusters, segment_plane, plane_inliers, estimate_normals, estimate_normals_radius, mask_by_confidence, read_ply, read_point_cloud, read_triangle_mesh, remove_radius_outlier,
                         remove_statistical_outlier, triangulate_points,
                         triangulate_points_with_normals, valid_points, voxel_down_sample, write_ply, write_point_cloud,
                         write_triangle_mesh, registration_icp, evaluate_registration, transform_points,
                         TSDFVolume, camera_from_Q, invert_rigid)
from ._lib import SGM_OPT_CONFIDENCE, SGM_TAP_CONF, SGM_TAP_CONF_RAW
from ._lib import SGM_OPT_RIGHT_VIEW, SGM_TAP_RIGHT, SGM_TAP_RIGHT_RAW

__all__ = [
    "StereoSGBM_create", "StereoSGBM", "reprojectImageTo3D", "error", "Engine", "get_engine", "set_device",
    "get_device", "clear_engine_cache", "compute_disparity_map", "reconstruct_3D", "valid_point_mask",
    "run_disparity", "valid_points", "write_point_cloud", "read_point_cloud", "STEREO_SGBM_MODE_SGBM", "STEREO_SGBM_MODE_HH", "STEREO_SGBM_MODE_SGBM_3WAY",
    "STEREO_SGBM_MODE_HH4", "CV_32F", "CV_32FC1", "INTER_LINEAR", "BORDER_CONSTANT", "initUndistortRectifyMap", "remap", "rectify_pair",
    "mask_by_confidence", "SGM_OPT_CONFIDENCE", "SGM_TAP_CONF_RAW", "SGM_TAP_CONF",
    "SGM_OPT_RIGHT_VIEW", "SGM_TAP_RIGHT_RAW", "SGM_TAP_RIGHT", "STEREO_COST_BT", "STEREO_COST_CENSUS",
    "DisparityWLSFilter", "createDisparityWLSFilter", "wls_weights", "lrcConfidence",
    "voxel_down_sample", "triangulate_points", "write_triangle_mesh", "read_triangle_mesh",
    "estimate_normals", "triangulate_points_with_normals", "write_ply", "read_ply",
    "remove_radius_outlier", "remove_statistical_outlier", "estimate_normals_radius",
    "cluster_dbscan", "largest_clusters", "segment_plane", "plane_inliers",
    "registration_icp", "evaluate_registration", "transform_points",
    "TSDFVolume", "camera_from_Q", "invert_rigid",
]
