"""Consumers of the XYZ image on the reference's path.

    valid_points(points_3D, colors, disparity_map)   main.ipynb:726-737  mask + boolean indexing
                 [, confidence, min_confidence]        ... and confidence >= min_confidence (StereoSGBM.computeWithConfidence)
    write_point_cloud(path, points, colors)           main.ipynb:795-797  o3d.io.write_point_cloud(.ply)
    voxel_down_sample(points_3D, colors, disparity_map, voxel_size, ...)   what users thin the cloud with before they show or
                 ship it: one centroid, mean colour and count per voxel, on the GPU (include/sgm_hip_voxel.h; NOT Open3D's values or order)
    remove_radius_outlier(points_3D, colors, disparity_map, nb_points, radius, ...)   the first thing users do to a stereo cloud:
                 drop the points with fewer than nb_points others within radius, on the GPU (include/sgm_hip_radius.h; NOT Open3D's)
    remove_statistical_outlier(points_3D, colors, disparity_map, nb_neighbors, std_ratio, max_radius, ...)   its companion: drop the
                 points whose mean distance to their nb_neighbors nearest others within max_radius is above the cloud's own mean of
                 it plus std_ratio deviations, on the GPU (include/sgm_hip_statistical.h; NOT Open3D's)
    triangulate_points(points_3D, colors, disparity_map, max_diff, ...)    the surface over the organised cloud: two triangles per
                 pixel quad wherever the disparity is continuous, on the GPU (include/sgm_hip_mesh.h; NOT Open3D's meshing)
    write_triangle_mesh(path, vertices, triangles, colors)                 its PLY export, in the layout of Open3D's mesh writer
    estimate_normals(points_3D, disparity_map, max_diff, ...)              one unit normal per pixel of the organised cloud, and
    triangulate_points_with_normals(points_3D, colors, disparity_map, ...) the mesh with one per vertex: the area-weighted sum of the
                 triangles around it, on the GPU (include/sgm_hip_normals.h; NOT Open3D's estimate_normals / compute_vertex_normals)
    estimate_normals_radius(points_3D, disparity_map, radius, ...)         one unit normal per point of a point LIST (voxel centroids,
                 a cleaned list, a cloud read back): the plane fitted to the neighbours within radius, on the GPU
                 (include/sgm_hip_covariance.h; NOT Open3D's estimate_normals)
    cluster_dbscan(points_3D, disparity_map, eps, min_points, ...)         the cloud split into the objects it holds: a cluster number
                 per point or -1 for noise, on the GPU (include/sgm_hip_dbscan.h; NOT Open3D's cluster_dbscan), and
    largest_clusters(labels, sizes, count, min_size)                       the mask of the largest of them, usable as a confidence map
    segment_plane(points_3D, colors, disparity_map, distance_threshold, ...)   the dominant plane of the cloud (floor, table, wall)
                 and the mask of the points on it, or with invert=True off it, on the GPU (include/sgm_hip_plane.h; NOT Open3D's
                 segment_plane), and
    plane_inliers(points_3D, colors, disparity_map, plane_model, distance_threshold, ...)   a model found once applied to other clouds
    registration_icp(source, target, max_correspondence_distance, ...)     the rigid motion that lays one cloud on another, by
                 iterated closest points on the GPU (include/sgm_hip_icp.h; NOT Open3D's registration_icp), with
    evaluate_registration(source, target, max_correspondence_distance, transformation)   its correspondence pass alone, and
    transform_points(points, transformation, normals)                      the motion applied, so that the two can be merged
    TSDFVolume(voxel_size, sdf_trunc, dims, ...).integrate(...) / .extract_point_cloud()   many frames with their poses fused into
                 one denoised surface: a dense signed distance volume of integer sums on the GPU (include/sgm_hip_tsdf.h; NOT
                 Open3D's UniformTSDFVolume), with camera_from_Q(Q) and invert_rigid(T) for its camera and pose
    write_ply(path, points, colors, normals, triangles) / read_ply(path)   one PLY writer for a cloud or a mesh, with or without normals

The compaction runs on the GPU (ordered, so the result equals numpy's `points_3D[mask]`); the
PLY writer is plain host I/O and replaces the Open3D dependency (absent here) for export only --
interactive viewing (o3d.visualization.draw_geometries) is out of scope.
"""
from __future__ import annotations

import numpy as np

from . import stereo as _cv


def mask_by_confidence(disparity_map, confidence, min_confidence):
    """The disparity map with 0 wherever confidence < min_confidence (a copy; 0 fails the `disparity_map > 0` of the
    notebook's mask), so that the existing compaction drops those pixels too."""
    disp = np.asarray(disparity_map)
    conf = np.asarray(confidence)
    if conf.shape != disp.shape:
        raise _cv.error("valid_points: confidence must have the shape of disparity_map")
    return np.where(conf >= min_confidence, disp, disp.dtype.type(0))


def valid_points(points_3D, colors, disparity_map, confidence=None, min_confidence=0):
    """Returns (valid_points float32 (N,3), valid_colors uint8 (N,3) or None) exactly like
    `points_3D[mask]`, `colors[mask]` with mask = ~isnan(X) & ~isinf(X) & (disparity_map > 0).
    With a confidence map (StereoSGBM.computeWithConfidence) the mask also requires confidence >= min_confidence."""
    pts = np.asarray(points_3D)
    disp = np.asarray(disparity_map)
    if pts.ndim != 3 or pts.shape[2] != 3 or pts.shape[:2] != disp.shape:
        raise _cv.error("valid_points: points_3D must be (H, W, 3) and disparity_map (H, W)")
    if confidence is not None:
        disp = mask_by_confidence(disp, confidence, min_confidence)
    if colors is not None:
        colors = np.asarray(colors)
        if colors.shape != pts.shape:
            raise _cv.error("valid_points: colors must have the shape of points_3D")
    return _cv.get_engine(_cv._DEFAULT).compact_points_host(pts, disp, colors)


VOXEL_MAX_POINTS = (1 << 24) - 1


def voxel_down_sample(points_3D, colors, disparity_map, voxel_size, origin=(0, 0, 0), min_points=1, confidence=None,
                      min_confidence=0, return_counts=False):
    """Voxel-grid downsampling on the GPU: one centroid, one mean colour and one count per occupied voxel of the grid of cubes of
    edge voxel_size anchored at origin; voxels with fewer than min_points points are dropped (a cheap outlier filter), and the
    voxels come in the order of their first points.  The definition is include/sgm_hip_voxel.h, our own and in integers, so the
    result is the same bits on every run: it is NOT Open3D's voxel_down_sample, neither in its values nor in its order.
    points_3D (H, W, 3) with disparity_map (H, W) -- a point counts iff X, Y, Z are finite and its disparity > 0, and with a
    confidence map also confidence >= min_confidence, as in valid_points -- or an (N, 3) list with disparity_map=None (every
    finite point counts).  colors: uint8 of the shape of points_3D, or None.
    Returns (points float32 (M, 3), colors uint8 (M, 3) or None[, counts uint32 (M)])."""
    who = "voxel_down_sample"
    pts, disp, colors = _outlier_cloud(who, points_3D, colors, disparity_map, confidence, min_confidence)
    with np.errstate(all="ignore"):
        try:
            v = np.float32(voxel_size)
            org = np.asarray(origin, np.float32)
        except (TypeError, ValueError):
            raise _cv.error(f"{who}: voxel_size and origin must be numbers") from None
        if v.shape != () or not np.isfinite(v) or not v > 0 or not np.isfinite(np.float32(1.0) / v):
            raise _cv.error(f"{who}: voxel_size={voxel_size!r} is not a finite positive float32 with a finite reciprocal")
    if org.shape != (3,) or not np.isfinite(org).all():
        raise _cv.error(f"{who}: origin={origin!r} is not three finite numbers")
    _int_arg(who, min_points, 1, 2 ** 31 - 1, f"min_points={min_points!r} is not an integer >= 1")
    if pts.size // 3 > VOXEL_MAX_POINTS:
        raise _cv.error(f"{who}: {pts.size // 3} points, more than {VOXEL_MAX_POINTS} (include/sgm_hip_voxel.h)")
    if pts.size == 0:      # nothing to send to the device
        none = np.zeros((0, 3), np.float32), None if colors is None else np.zeros((0, 3), np.uint8)
        return none + (np.zeros(0, np.uint32),) if return_counts else none
    p, c, k, _ = _cv.get_engine(_cv._DEFAULT).voxel_downsample_host(pts, disp, colors, float(v), org, int(min_points),
                                                                   bool(return_counts))
    return (p, c, k) if return_counts else (p, c)


RADIUS_MAX_POINTS = (1 << 24) - 1


def _int_arg(who, v, lo, hi, message):
    """an argument that must be an integer (no bool) in lo .. hi, or the error `who: message`"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise _cv.error(f"{who}: {message}")


def _outlier_cloud(who, points_3D, colors, disparity_map, confidence, min_confidence):
    """what the calls on arrays accept as a cloud: (points, disparities or None, colours or None), checked"""
    pts = np.asarray(points_3D)
    if pts.dtype != np.float32:
        raise _cv.error(f"{who}: points_3D must be float32, not {pts.dtype}")
    if disparity_map is None:
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise _cv.error(f"{who}: without a disparity_map points_3D must be an (N, 3) list")
        if confidence is not None:
            raise _cv.error(f"{who}: a confidence map needs a disparity_map")
        disp = None
    else:
        disp = np.asarray(disparity_map)
        if pts.ndim != 3 or pts.shape[2] != 3 or pts.shape[:2] != disp.shape:
            raise _cv.error(f"{who}: points_3D must be (H, W, 3) and disparity_map (H, W)")
        if confidence is not None:
            disp = mask_by_confidence(disp, confidence, min_confidence)
    if colors is not None:
        colors = np.asarray(colors)
        if colors.shape != pts.shape or colors.dtype != np.uint8:
            raise _cv.error(f"{who}: colors must be uint8 and have the shape of points_3D")
    return pts, disp, colors


def _search_radius(who, name, radius, origin, extra_scales=(), numbers=None):
    """what the searches on the grid of cells accept as their radius (`name` is the caller's word for it) and origin, checked
    in the engine's float32 arithmetic: (np.float32 r, float32 origin[3]).  extra_scales: the s whose s / r must stay finite as
    well; numbers: what the 'must be numbers' message names, where that is more than these two"""
    with np.errstate(all="ignore"):
        try:
            r = np.float32(radius)
            org = np.asarray(origin, np.float32)
        except (TypeError, ValueError):
            raise _cv.error(f"{who}: {numbers or name + ' and origin'} must be numbers") from None
        r2 = r * r
        if (r.shape != () or not np.isfinite(r) or not r > 0 or not np.isfinite(r2) or r2 < np.finfo(np.float32).tiny
                or not np.isfinite(np.float32(1.0) / (r * np.float32(1.03125)))
                or not all(np.isfinite(np.float32(s) / r) for s in extra_scales)):
            raise _cv.error(f"{who}: {name}={radius!r} is not a finite positive float32 with a finite normal square")
    if org.shape != (3,) or not np.isfinite(org).all():
        raise _cv.error(f"{who}: origin={origin!r} is not three finite numbers")
    return r, org


def remove_radius_outlier(points_3D, colors, disparity_map, nb_points, radius, origin=(0, 0, 0), max_count=None, confidence=None,
                          min_confidence=0, return_mask=False, return_counts=False, return_index=False):
    """Radius outlier removal on the GPU: keeps the points that have at least nb_points OTHER points within radius, in source
    order.  The definition is include/sgm_hip_radius.h, our own, and the result is the same bits on every run: it is NOT Open3D's
    remove_radius_outlier -- a point does not count itself, points whose cell index (cells of edge radius * 1.03125 anchored at
    origin) leaves -2^16 .. 2^16 - 1 are dropped, and the counts saturate at max_count (None: nb_points), where a point's search
    stops.  A fixed metric radius thins the far range of a stereo cloud, whose point spacing grows with depth.
    points_3D (H, W, 3) with disparity_map (H, W) -- a point takes part iff X, Y, Z are finite and its disparity > 0, and with a
    confidence map also confidence >= min_confidence, as in valid_points -- or an (N, 3) list with disparity_map=None (every
    finite point takes part).  colors: uint8 of the shape of points_3D, or None.
    Returns (points float32 (M, 3), colors uint8 (M, 3) or None[, mask][, counts][, index]): mask uint8, 1 where the point is
    kept -- usable as the `confidence` of valid_points, triangulate_points and estimate_normals with min_confidence=1 -- and
    counts uint32, min(neighbours, max_count), both of the shape of disparity_map (of (N,) for a list); index uint32 (M), the
    source index of each kept point."""
    who = "remove_radius_outlier"
    pts, disp, colors = _outlier_cloud(who, points_3D, colors, disparity_map, confidence, min_confidence)
    r, org = _search_radius(who, "radius", radius, origin)
    _int_arg(who, nb_points, 1, 2 ** 31 - 1, f"nb_points={nb_points!r} is not an integer >= 1")
    if max_count is not None:
        _int_arg(who, max_count, int(nb_points), 2 ** 31 - 1, f"max_count={max_count!r} is not an integer >= nb_points")
    n = pts.size // 3
    if n > RADIUS_MAX_POINTS:
        raise _cv.error(f"{who}: {n} points, more than {RADIUS_MAX_POINTS} (include/sgm_hip_radius.h)")
    shape = pts.shape[:-1]
    if n == 0:      # nothing to send to the device
        p, c, keep, cnt, idx = (np.zeros((0, 3), np.float32), None if colors is None else np.zeros((0, 3), np.uint8),
                                np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    else:
        p, c, keep, cnt, idx, _ = _cv.get_engine(_cv._DEFAULT).radius_outlier_host(
            pts, disp, colors, float(r), int(nb_points), None if max_count is None else int(max_count), org, bool(return_counts),
            bool(return_index))
    out = (p, c)
    if return_mask:
        out += (keep.reshape(shape),)
    if return_counts:
        out += (cnt.reshape(shape),)
    if return_index:
        out += (idx,)
    return out


STATISTICAL_MAX_NEIGHBORS = 64


def remove_statistical_outlier(points_3D, colors, disparity_map, nb_neighbors, std_ratio, max_radius, origin=(0, 0, 0), confidence=None,
                               min_confidence=0, return_mask=False, return_distances=False, return_index=False, return_stats=False):
    """Statistical outlier removal on the GPU: per point the mean distance to its nb_neighbors nearest OTHER points within
    max_radius, and the points whose mean is not above the cloud's mean of these means plus std_ratio standard deviations, in
    source order.  The definition is include/sgm_hip_statistical.h, our own, and the result is the same bits on every run: it is
    NOT Open3D's remove_statistical_outlier -- the search is bounded by max_radius and a point with fewer than nb_neighbors
    (1 .. 64) neighbours there is an outlier outright and stays out of the statistic, a point does not count itself, points whose
    cell index (cells of edge max_radius * 1.03125 anchored at origin) leaves -2^16 .. 2^16 - 1 are dropped, and the statistic is
    formed in integers (the means scaled by 2^19 / max_radius).  max_radius should hold a few times nb_neighbors neighbours; the
    work grows with every candidate in the 27 cells around a point.  A fixed metric max_radius thins the far range of a stereo
    cloud, whose point spacing grows with depth.
    points_3D (H, W, 3) with disparity_map (H, W) -- a point takes part iff X, Y, Z are finite and its disparity > 0, and with a
    confidence map also confidence >= min_confidence, as in valid_points -- or an (N, 3) list with disparity_map=None (every
    finite point takes part).  colors: uint8 of the shape of points_3D, or None.
    Returns (points float32 (M, 3), colors uint8 (M, 3) or None[, mask][, distances][, index][, stats]): mask uint8, 1 where the
    point is kept -- usable as the `confidence` of valid_points, triangulate_points and estimate_normals with min_confidence=1 --
    and distances float32, the mean distance of a point with nb_neighbors neighbours and -1 for every other point, both of the
    shape of disparity_map (of (N,) for a list); index uint32 (M), the source index of each kept point; stats a dict: in_range,
    out_of_range, dense, sparse, A, B, T."""
    who = "remove_statistical_outlier"
    pts, disp, colors = _outlier_cloud(who, points_3D, colors, disparity_map, confidence, min_confidence)
    _int_arg(who, nb_neighbors, 1, STATISTICAL_MAX_NEIGHBORS, f"nb_neighbors={nb_neighbors!r} is not an integer in 1 .. {STATISTICAL_MAX_NEIGHBORS}")
    with np.errstate(all="ignore"):
        try:
            ratio = np.float32(std_ratio)
        except (TypeError, ValueError):
            raise _cv.error(f"{who}: std_ratio={std_ratio!r} is not a number") from None
        if isinstance(std_ratio, bool) or ratio.shape != () or not np.isfinite(ratio) or not ratio >= 0:
            raise _cv.error(f"{who}: std_ratio={std_ratio!r} is not a finite float32 >= 0")
    r, org = _search_radius(who, "max_radius", max_radius, origin, (524288.0,))
    n = pts.size // 3
    if n > RADIUS_MAX_POINTS:
        raise _cv.error(f"{who}: {n} points, more than {RADIUS_MAX_POINTS} (include/sgm_hip_statistical.h)")
    shape = pts.shape[:-1]
    if n == 0:      # nothing to send to the device
        p, c, keep, mean, idx, st = (np.zeros((0, 3), np.float32), None if colors is None else np.zeros((0, 3), np.uint8),
                                     np.zeros(0, np.uint8), np.zeros(0, np.float32), np.zeros(0, np.uint32), np.zeros(8, np.uint64))
    else:
        p, c, keep, mean, idx, st = _cv.get_engine(_cv._DEFAULT).statistical_outlier_host(
            pts, disp, colors, int(nb_neighbors), float(ratio), float(r), org, bool(return_distances), bool(return_index))
    out = (p, c)
    if return_mask:
        out += (keep.reshape(shape),)
    if return_distances:
        out += (mean.reshape(shape),)
    if return_index:
        out += (idx,)
    if return_stats:
        out += (dict(zip(("in_range", "out_of_range", "dense", "sparse", "A", "B", "T"), (int(x) for x in st[:7]))),)
    return out


COVARIANCE_MIN_NEIGHBORS = 2
COVARIANCE_STATS = ("in_range", "out_of_range", "with_normal", "degenerate")


def estimate_normals_radius(points_3D, disparity_map, radius, min_neighbors=3, origin=(0, 0, 0), viewpoint=(0, 0, 0), orient=True,
                            confidence=None, min_confidence=0, return_curvature=False, return_counts=False, return_stats=False):
    """Covariance (PCA) normals for a point LIST, on the GPU: per point the unit normal of the plane fitted to its OTHER points
    within radius -- the eigenvector of the smallest eigenvalue of their covariance --, and with orient turned towards viewpoint.
    A point with fewer than min_neighbors (>= 2) neighbours, or whose neighbours all sit on it, gets (0, 0, 0).  Where
    estimate_normals needs the pixel grid, this needs points only: the centroids of voxel_down_sample, a list cleaned by
    remove_radius_outlier or remove_statistical_outlier, a cloud from read_ply, two clouds concatenated.  The definition is
    include/sgm_hip_covariance.h, our own, and the result is the same bits on every run: it is NOT Open3D's estimate_normals --
    a point is not its own neighbour, points whose cell index (cells of edge radius * 1.03125 anchored at origin) leaves
    -2^16 .. 2^16 - 1 get no normal, the neighbours' offsets are quantised to radius / 32768 and summed in integers, and the 3 x 3
    eigenproblem is solved by six fixed Jacobi sweeps in binary64.  The radius should hold ten to a few tens of neighbours; the
    work grows with every candidate in the 27 cells around a point.
    points_3D (H, W, 3) with disparity_map (H, W) -- a point takes part iff X, Y, Z are finite and its disparity > 0, and with a
    confidence map also confidence >= min_confidence, as in valid_points -- or an (N, 3) list with disparity_map=None (every
    finite point takes part); numpy arrays, or HIP tensors (float32, on the GPU), which stay on the device.
    Returns normals float32 of the shape of points_3D, or with any of the return_ flags a tuple (normals[, curvature][, counts]
    [, stats]): curvature float32, the surface variation l_min / (l_0 + l_1 + l_2) in 0 .. 1/3 and -1 where there is no normal;
    counts uint32 (int32 for tensors), the number of neighbours; both of the shape of disparity_map (of (N,) for a list); stats a
    dict: in_range, out_of_range, with_normal, degenerate.

    The chain this exists for:

        centroids, colors = voxel_down_sample(points_3D, colors, disparity_map, voxel_size)
        normals = estimate_normals_radius(centroids, None, radius=2 * voxel_size)
        write_ply(path, centroids, colors, normals)
    """
    who = "estimate_normals_radius"
    on_device, pts, disp, _, shape, n = _host_or_device_cloud(who, points_3D, None, disparity_map, confidence, min_confidence)
    numbers = "radius, origin and viewpoint"
    try:
        with np.errstate(all="ignore"):
            view = np.asarray(viewpoint, np.float32)
    except (TypeError, ValueError):
        raise _cv.error(f"{who}: {numbers} must be numbers") from None
    r, org = _search_radius(who, "radius", radius, origin, (32768.0,), numbers)
    if view.shape != (3,) or not np.isfinite(view).all():
        raise _cv.error(f"{who}: viewpoint={viewpoint!r} is not three finite numbers")
    _int_arg(who, min_neighbors, COVARIANCE_MIN_NEIGHBORS, RADIUS_MAX_POINTS,
             f"min_neighbors={min_neighbors!r} is not an integer in {COVARIANCE_MIN_NEIGHBORS} .. {RADIUS_MAX_POINTS}")
    if not isinstance(orient, (bool, np.bool_)):
        raise _cv.error(f"{who}: orient={orient!r} is not a bool")
    if n > RADIUS_MAX_POINTS:
        raise _cv.error(f"{who}: {n} points, more than {RADIUS_MAX_POINTS} (include/sgm_hip_covariance.h)")
    if on_device:
        import torch
        nrm = torch.zeros(shape + (3,), dtype=torch.float32, device=pts.device)
        curv = torch.full(shape, -1.0, dtype=torch.float32, device=pts.device) if return_curvature else None
        cnt = torch.zeros(shape, dtype=torch.int32, device=pts.device) if return_counts else None     # (the bits of uint32 counts < 2^24)
        st = np.zeros(4, np.uint64)
        if n:
            e = _cv.get_engine(_cv._DEFAULT, pts.device.index)
            torch.cuda.synchronize(pts.device)      # the inputs were made on torch's stream, the call runs on the engine's
            ptr = lambda t: None if t is None else t.data_ptr()
            st = e.covariance_normals_device(pts.data_ptr(), ptr(disp), n, float(r), int(min_neighbors), org, view, bool(orient),
                                             nrm.data_ptr(), ptr(curv), ptr(cnt))
    elif n == 0:      # nothing to send to the device
        nrm, curv, cnt, st = (np.zeros(shape + (3,), np.float32), np.zeros(shape, np.float32), np.zeros(shape, np.uint32),
                              np.zeros(4, np.uint64))
    else:
        nrm, curv, cnt, st = _cv.get_engine(_cv._DEFAULT).covariance_normals_host(
            pts, disp, float(r), int(min_neighbors), org, view, bool(orient), bool(return_curvature), bool(return_counts))
        nrm = nrm.reshape(shape + (3,))
        curv = None if curv is None else curv.reshape(shape)
        cnt = None if cnt is None else cnt.reshape(shape)
    out = (nrm,)
    if return_curvature:
        out += (curv,)
    if return_counts:
        out += (cnt,)
    if return_stats:
        out += (dict(zip(COVARIANCE_STATS, (int(x) for x in st))),)
    return out if len(out) > 1 else nrm


def _device_cloud(who, points_3D, disparity_map, confidence, min_confidence):
    """what estimate_normals_radius accepts as a cloud on the device: (points, disparities or None) as contiguous float32 HIP
    tensors, the confidence mask applied to a copy of the disparities"""
    import torch
    pts = points_3D
    if not pts.is_cuda or pts.dtype != torch.float32:
        raise _cv.error(f"{who}: a tensor points_3D must be float32 and on the GPU")
    if disparity_map is None:
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise _cv.error(f"{who}: without a disparity_map points_3D must be an (N, 3) list")
        if confidence is not None:
            raise _cv.error(f"{who}: a confidence map needs a disparity_map")
        return pts.contiguous(), None
    disp = disparity_map
    if not _cv._is_torch(disp) or disp.device != pts.device or disp.dtype != torch.float32:
        raise _cv.error(f"{who}: with a tensor points_3D the disparity_map must be a float32 tensor on the same GPU")
    if pts.dim() != 3 or pts.shape[2] != 3 or pts.shape[:2] != disp.shape:
        raise _cv.error(f"{who}: points_3D must be (H, W, 3) and disparity_map (H, W)")
    if confidence is not None:
        conf = confidence if _cv._is_torch(confidence) else torch.from_numpy(np.ascontiguousarray(confidence))
        if tuple(conf.shape) != tuple(disp.shape):
            raise _cv.error(f"{who}: confidence must have the shape of disparity_map")
        disp = torch.where(conf.to(pts.device) >= min_confidence, disp, torch.zeros_like(disp))
    return pts.contiguous(), disp.contiguous()


def _host_or_device_cloud(who, points_3D, colors, disparity_map, confidence, min_confidence):
    """the cloud of a call that takes arrays or tensors, checked: (on_device, points, disparities or None, colours -- of a tensor
    cloud as given --, the shape of the per-point results, n)"""
    if _cv._is_torch(points_3D):
        pts, disp = _device_cloud(who, points_3D, disparity_map, confidence, min_confidence)
        return True, pts, disp, colors, tuple(pts.shape[:-1]), pts.numel() // 3
    pts, disp, colors = _outlier_cloud(who, points_3D, colors, disparity_map, confidence, min_confidence)
    return False, pts, disp, colors, pts.shape[:-1], pts.size // 3


DBSCAN_STATS = ("in_range", "out_of_range", "core", "border", "noise", "clusters")


def cluster_dbscan(points_3D, disparity_map, eps, min_points, origin=(0, 0, 0), confidence=None, min_confidence=0, return_core=False,
                   return_sizes=False, return_stats=False):
    """Density clustering of the cloud, on the GPU: per point the number of the cluster it belongs to, or -1 for noise.  A point
    with at least min_points OTHER points within eps is a core point; core points within eps of each other are one cluster; a
    point that is not core but has a core point within eps is a border point and joins the cluster of its nearest core point (ties
    in the binary32 squared distance go to the lowest index); everything else is noise.  The clusters are numbered 0, 1, ... by
    the smallest index among their core points.  The definition is include/sgm_hip_dbscan.h, our own, and the result is the same
    bits on every run and does not depend on the order of the points beyond the numbering: it is NOT Open3D's cluster_dbscan
    (nor scikit-learn's DBSCAN) -- a point does not count itself, so Open3D's min_points is ours plus one; points whose cell index
    (cells of edge eps * 1.03125 anchored at origin) leaves -2^16 .. 2^16 - 1 are noise; and a border point goes to its nearest
    core point, not to whichever cluster reaches it first.  The work grows with every candidate in the 27 cells around a point: thin
    the cloud first and cluster at about twice the voxel size.
    points_3D (H, W, 3) with disparity_map (H, W) -- a point takes part iff X, Y, Z are finite and its disparity > 0, and with a
    confidence map also confidence >= min_confidence, as in valid_points -- or an (N, 3) list with disparity_map=None (every
    finite point takes part); numpy arrays, or HIP tensors (float32, on the GPU), which stay on the device.
    Returns labels int32 of the shape of disparity_map (of (N,) for a list), or with any of the return_ flags a tuple (labels[,
    core][, sizes][, stats]): core uint8 of the same shape, 1 for a core point; sizes uint32 (int32 for tensors) (clusters,), the
    core and border points of each cluster; stats a dict: in_range, out_of_range, core, border, noise (in range), clusters.

    The chain this exists for:

        centroids, colors = voxel_down_sample(points_3D, colors, disparity_map, voxel_size)
        labels, sizes = cluster_dbscan(centroids, None, eps=2 * voxel_size, min_points=4, return_sizes=True)
        mask = largest_clusters(labels, sizes)
        statue, statue_colors = centroids[mask > 0], colors[mask > 0]

    In short voxel_down_sample -> cluster_dbscan -> largest_clusters -> valid_points: on the organised cloud itself the labels
    of cluster_dbscan(points_3D, disparity_map, eps, min_points) have the shape of the disparity map, and the mask goes into
    valid_points(points_3D, colors, disparity_map, confidence=mask, min_confidence=1).
    """
    who = "cluster_dbscan"
    on_device, pts, disp, _, shape, n = _host_or_device_cloud(who, points_3D, None, disparity_map, confidence, min_confidence)
    r, org = _search_radius(who, "eps", eps, origin)
    _int_arg(who, min_points, 1, RADIUS_MAX_POINTS, f"min_points={min_points!r} is not an integer in 1 .. {RADIUS_MAX_POINTS}")
    if n > RADIUS_MAX_POINTS:
        raise _cv.error(f"{who}: {n} points, more than {RADIUS_MAX_POINTS} (include/sgm_hip_dbscan.h)")
    if on_device:
        import torch
        labels = torch.full(shape, -1, dtype=torch.int32, device=pts.device)
        core = torch.zeros(shape, dtype=torch.uint8, device=pts.device) if return_core else None
        sizes = torch.zeros(n, dtype=torch.int32, device=pts.device) if return_sizes else None      # (the bits of uint32 sizes < 2^24)
        nc, st = 0, np.zeros(6, np.uint64)
        if n:
            e = _cv.get_engine(_cv._DEFAULT, pts.device.index)
            torch.cuda.synchronize(pts.device)      # the inputs were made on torch's stream, the call runs on the engine's
            ptr = lambda t: None if t is None else t.data_ptr()
            nc, st = e.cluster_dbscan_device(pts.data_ptr(), ptr(disp), n, float(r), int(min_points), org, labels.data_ptr(), ptr(core),
                                             ptr(sizes))
        sizes = None if sizes is None else sizes[:nc].clone()
    elif n == 0:      # nothing to send to the device
        labels, core, sizes, st = np.zeros(shape, np.int32), np.zeros(shape, np.uint8), np.zeros(0, np.uint32), np.zeros(6, np.uint64)
    else:
        labels, core, sizes, st = _cv.get_engine(_cv._DEFAULT).cluster_dbscan_host(pts, disp, float(r), int(min_points), org,
                                                                                   bool(return_core), bool(return_sizes))
        labels = labels.reshape(shape)
        core = None if core is None else core.reshape(shape)
    out = (labels,)
    if return_core:
        out += (core,)
    if return_sizes:
        out += (sizes,)
    if return_stats:
        out += (dict(zip(DBSCAN_STATS, (int(x) for x in st))),)
    return out if len(out) > 1 else labels


def largest_clusters(labels, sizes, count=1, min_size=1):
    """The points of the `count` largest clusters of cluster_dbscan that have at least min_size points, as a uint8 mask of the shape
    of labels: 1 where the point's label is one of them, 0 elsewhere (noise included).  Among clusters of the same size the lower
    label is the larger.  The mask is usable as the `confidence` of valid_points, triangulate_points, estimate_normals and the
    outlier removals with min_confidence=1.  Plain numpy, or plain torch for tensors: no kernel."""
    who = "largest_clusters"
    for name, v in (("count", count), ("min_size", min_size)):
        lo = 0 if name == "count" else 1
        _int_arg(who, v, lo, float("inf"), f"{name}={v!r} is not an integer >= {lo}")
    if _cv._is_torch(labels):
        import torch
        sz = sizes if _cv._is_torch(sizes) else torch.from_numpy(np.asarray(sizes).astype(np.int64))
        sz = sz.to(labels.device).to(torch.int64).reshape(-1)
        if labels.dtype != torch.int32:
            raise _cv.error(f"{who}: labels must be int32")
        if labels.numel() and int(labels.max()) >= sz.numel():
            raise _cv.error(f"{who}: a label is not below the {sz.numel()} sizes")
        order = torch.argsort(-sz, stable=True)[:int(count)]      # descending size, ties in ascending label
        order = order[sz[order] >= int(min_size)]
        chosen = torch.zeros(sz.numel() + 1, dtype=torch.uint8, device=labels.device)      # (the last row is noise's)
        chosen[order] = 1
        lab = labels.to(torch.int64)
        return chosen[torch.where(lab >= 0, lab, torch.full_like(lab, sz.numel()))]
    lab = np.asarray(labels)
    sz = np.asarray(sizes).astype(np.int64).reshape(-1)
    if lab.dtype != np.int32:
        raise _cv.error(f"{who}: labels must be int32, not {lab.dtype}")
    if lab.size and int(lab.max()) >= sz.size:
        raise _cv.error(f"{who}: a label is not below the {sz.size} sizes")
    order = np.argsort(-sz, kind="stable")[:int(count)]
    order = order[sz[order] >= int(min_size)]
    chosen = np.zeros(sz.size + 1, np.uint8)
    chosen[order] = 1
    return chosen[np.where(lab >= 0, lab, sz.size)]


PLANE_STATS = ("valid", "degenerate", "best", "best_count", "refit_points", "out_of_refit_range", "refined", "found")
PLANE_MAX_ITERATIONS = 65536


def _plane_threshold(who, distance_threshold):
    """the distance threshold as the engine's float32, checked as step 2 of include/sgm_hip_plane.h checks it"""
    with np.errstate(all="ignore"):
        try:
            t = np.float32(distance_threshold)
        except (TypeError, ValueError):
            raise _cv.error(f"{who}: distance_threshold must be a number") from None
        if (t.shape != () or not np.isfinite(t) or not t > 0 or t < np.finfo(np.float32).tiny
                or not np.isfinite(np.float32(32.0) / t)):
            raise _cv.error(f"{who}: distance_threshold={distance_threshold!r} is not a finite positive normal float32 with a finite 32 / t")
    return t


def _plane_call(who, points_3D, colors, disparity_map, confidence, min_confidence, select, flags, host, device):
    """what segment_plane and plane_inliers share behind their argument checks: the cloud on the host or on the device, the call
    (host(engine, pts, disp, colors) or device(engine, pts, disp, colors, n, outputs...)), and the optional results in their order.
    Returns (head, mask, points, colors, index, distances): head is what the call returns in front of the per-point results."""
    return_points, return_index, return_distances = flags
    on_device, pts, disp, colors, shape, n = _host_or_device_cloud(who, points_3D, colors, disparity_map, confidence, min_confidence)
    if on_device:
        import torch
        if colors is not None and (not _cv._is_torch(colors) or colors.device != pts.device or colors.dtype != torch.uint8
                                   or tuple(colors.shape) != tuple(pts.shape)):
            raise _cv.error(f"{who}: with a tensor points_3D colors must be a uint8 tensor of its shape on the same GPU")
        colors = None if colors is None else colors.contiguous()
    if n > RADIUS_MAX_POINTS:
        raise _cv.error(f"{who}: {n} points, more than {RADIUS_MAX_POINTS} (include/sgm_hip_plane.h)")
    want_index = return_index or bool(select)      # (the inverted mask is made from the selected indices)
    if on_device:
        dev = pts.device
        inl = torch.zeros(shape, dtype=torch.uint8, device=dev)
        dist = torch.full(shape, float("nan"), dtype=torch.float32, device=dev) if return_distances else None
        p = torch.empty((n, 3), dtype=torch.float32, device=dev) if return_points else None
        c = torch.empty((n, 3), dtype=torch.uint8, device=dev) if return_points and colors is not None else None
        idx = torch.empty(n, dtype=torch.int32, device=dev) if want_index else None      # (the bits of uint32 indices < 2^24)
        head, ns = None, 0
        if n:
            e = _cv.get_engine(_cv._DEFAULT, dev.index)
            torch.cuda.synchronize(dev)      # the inputs were made on torch's stream, the call runs on the engine's
            ptr = lambda t: None if t is None else t.data_ptr()
            head, ns = device(e, pts.data_ptr(), ptr(disp), ptr(colors), n, inl.data_ptr(), ptr(dist), ptr(p), ptr(c), ptr(idx))
        p, c, idx = (None if a is None else a[:ns].clone() for a in (p, c, idx))
        mask = inl
        if select:
            mask = torch.zeros(n, dtype=torch.uint8, device=dev)
            mask[idx.to(torch.int64)] = 1
            mask = mask.reshape(shape)
    else:
        head = None
        inl, dist = np.zeros(shape, np.uint8), (np.full(shape, np.nan, np.float32) if return_distances else None)
        p = np.zeros((0, 3), np.float32) if return_points else None
        c = np.zeros((0, 3), np.uint8) if return_points and colors is not None else None
        idx = np.zeros(0, np.uint32) if want_index else None
        if n:      # (an empty cloud needs no engine)
            head, inl, dist, p, c, idx = host(_cv.get_engine(_cv._DEFAULT), pts, disp, colors, want_index)
            inl = inl.reshape(shape)
            dist = None if dist is None else dist.reshape(shape)
        mask = inl
        if select:
            mask = np.zeros(n, np.uint8)
            mask[idx] = 1
            mask = mask.reshape(shape)
    return head, mask, p, c, idx if return_index else None, dist


def _plane_results(first, mask, p, c, idx, dist, stats, flags):
    return_points, return_index, return_distances = flags
    out = first + (mask,)
    if return_points:
        out += (p, c)
    if return_index:
        out += (idx,)
    if return_distances:
        out += (dist,)
    if stats is not None:
        out += (stats,)
    return out if len(out) > 1 else out[0]


def segment_plane(points_3D, colors, disparity_map, distance_threshold, ransac_n=3, num_iterations=1000, seed=0, refine=True,
                  invert=False, confidence=None, min_confidence=0, return_points=False, return_index=False, return_distances=False,
                  return_stats=False):
    """Plane segmentation of the cloud, on the GPU: the dominant plane (floor, table, wall) as plane_model = (a, b, c, d) with
    a x + b y + c z + d = 0 and (a, b, c) a unit normal, and the mask of the points within distance_threshold of it.  num_iterations
    hypotheses, each through three valid points drawn by a counter-based hash of seed, are ALL scored on EVERY valid point; the one
    with the most inliers wins (ties: the lowest index); with refine its inliers are refitted by the covariance of integer moments
    (offsets from one of its points quantised to distance_threshold / 32, out to +-16384 thresholds); the cloud is classified with
    the refitted model; the normal points to the side of the origin, where the camera is, so the signed distances are heights
    above a floor.  The definition is include/sgm_hip_plane.h, our own, and the result is the same bits on every run: it is NOT
    Open3D's segment_plane -- no random state, no probability-based early stop, no ransac_n other than 3 -- and with fewer than
    three valid points or inliers no plane is found: the model is (0, 0, 0, 0) and the mask empty.
    points_3D (H, W, 3) with disparity_map (H, W) -- a point takes part iff X, Y, Z are finite and its disparity > 0, and with a
    confidence map also confidence >= min_confidence, as in valid_points -- or an (N, 3) list with disparity_map=None (every
    finite point takes part); numpy arrays, or HIP tensors (float32, on the GPU), which stay on the device.  colors: uint8 of the
    shape of points_3D, or None.
    Returns (plane_model float32 (4), mask[, points, colors][, index][, distances][, stats]): mask uint8 of the shape of
    disparity_map (of (N,) for a list), 1 on the inliers -- with invert=True on the valid points that are NOT inliers --, usable as
    the `confidence` of valid_points, cluster_dbscan and the other cloud calls with min_confidence=1; points float32 (M, 3),
    colors uint8 (M, 3) or None and index uint32 (int32 for tensors) (M,): the masked points in source order; distances float32 of
    the mask's shape, the signed distance of every valid point and NaN elsewhere; stats a dict: valid, degenerate (hypotheses),
    best, best_count, refit_points, out_of_refit_range, refined, found.

    The chain this exists for -- the objects standing on a floor:

        model, off_floor = segment_plane(points_3D, None, disparity_map, 0.02, invert=True)
        labels, sizes = cluster_dbscan(points_3D, disparity_map, eps, min_points, confidence=off_floor, min_confidence=1, return_sizes=True)
        objects = largest_clusters(labels, sizes, count=5)
        points, colors = valid_points(points_3D, colors, disparity_map, confidence=objects, min_confidence=1)

    In short segment_plane(..., invert=True) -> cluster_dbscan(confidence=mask) -> largest_clusters -> valid_points.  Repeated calls
    with the previous inverted mask as confidence peel plane after plane.  plane_inliers applies a model found once to other clouds.
    """
    who = "segment_plane"
    _int_arg(who, ransac_n, 3, 3, f"ransac_n={ransac_n!r}: only 3 is offered (include/sgm_hip_plane.h)")
    t = _plane_threshold(who, distance_threshold)
    _int_arg(who, num_iterations, 1, PLANE_MAX_ITERATIONS, f"num_iterations={num_iterations!r} is not an integer in 1 .. {PLANE_MAX_ITERATIONS}")
    _int_arg(who, seed, 0, 2 ** 32 - 1, f"seed={seed!r} is not an integer in 0 .. 2^32 - 1")
    K, seed, refine, select = int(num_iterations), int(seed), bool(refine), int(bool(invert))
    flags = (bool(return_points), bool(return_index), bool(return_distances))

    def host(e, pts, disp, col, want_index):
        model, inl, dist, p, c, idx, st, _ = e.segment_plane_host(pts, disp, col, float(t), K, seed, refine, select, flags[2], flags[0],
                                                                  want_index)
        return (model, st), inl, dist, p, c, idx

    def device(e, d_xyz, d_disp, d_col, n, d_inl, d_dist, d_p, d_c, d_idx):
        model, st, _, ns = e.segment_plane_device(d_xyz, d_disp, d_col, n, float(t), K, seed, refine, select, d_inl, d_dist, d_p, d_c, d_idx)
        return (model, st), ns

    head, mask, p, c, idx, dist = _plane_call(who, points_3D, colors, disparity_map, confidence, min_confidence, select, flags, host, device)
    model, st = head if head is not None else (np.zeros(4, np.float32), np.zeros(8, np.uint64))
    stats = dict(zip(PLANE_STATS, (int(x) for x in st))) if return_stats else None
    return _plane_results((model,), mask, p, c, idx, dist, stats, flags)


def plane_inliers(points_3D, colors, disparity_map, plane_model, distance_threshold, invert=False, confidence=None, min_confidence=0,
                  return_points=False, return_index=False, return_distances=False):
    """The classification of segment_plane alone, on the GPU, with the caller's plane_model (a, b, c, d) -- a fixed rig fits its floor
    once and applies it to every frame: the mask of the valid points with |a x + b y + c z + d| <= distance_threshold, the sum as
    three binary32 fused multiply-adds from d (include/sgm_hip_plane.h, step 8; NOT Open3D's select_by_index on its own inliers).
    plane_model: four finite numbers whose (a, b, c) has a squared length within 2^-10 of 1 in float32.  The cloud, colors,
    confidence, invert and the return_ flags are segment_plane's.
    Returns mask, or with any of the return_ flags a tuple (mask[, points, colors][, index][, distances])."""
    who = "plane_inliers"
    with np.errstate(all="ignore"):
        try:
            model = np.asarray(plane_model.cpu() if _cv._is_torch(plane_model) else plane_model, np.float32)
        except (TypeError, ValueError):
            raise _cv.error(f"{who}: plane_model must be four numbers") from None
        ok = model.shape == (4,) and np.isfinite(model).all()
        if ok:
            len2 = (model[0] * model[0] + model[1] * model[1]) + model[2] * model[2]
            ok = bool(np.abs(len2 - np.float32(1)) <= np.float32(2.0 ** -10))
    if not ok:
        raise _cv.error(f"{who}: plane_model={plane_model!r} is not four finite numbers with a unit normal")
    t = _plane_threshold(who, distance_threshold)
    select = int(bool(invert))
    flags = (bool(return_points), bool(return_index), bool(return_distances))

    def host(e, pts, disp, col, want_index):
        inl, dist, p, c, idx, _ = e.plane_inliers_host(pts, disp, col, model, float(t), select, flags[2], flags[0], want_index)
        return None, inl, dist, p, c, idx

    def device(e, d_xyz, d_disp, d_col, n, d_inl, d_dist, d_p, d_c, d_idx):
        _, ns = e.plane_inliers_device(d_xyz, d_disp, d_col, n, model, float(t), select, d_inl, d_dist, d_p, d_c, d_idx)
        return None, ns

    _, mask, p, c, idx, dist = _plane_call(who, points_3D, colors, disparity_map, confidence, min_confidence, select, flags, host, device)
    return _plane_results((), mask, p, c, idx, dist, None, flags)


ICP_STATS = ("valid_source", "target_in_range", "target_out_of_range", "iterations", "correspondences", "unplaced", "unusable_normals",
             "status")
ICP_STATUS = ("converged", "max_iteration", "too_few", "degenerate")
ICP_ESTIMATIONS = ("point_to_point", "point_to_plane")
ICP_MAX_ITERATION = 1000


def _icp_matrix(who, name, T):
    """a rigid transformation as float64 (4, 4), checked as include/sgm_hip_icp.h checks it; None is the identity"""
    if T is None:
        return np.eye(4, dtype=np.float64)
    try:
        M = np.asarray(T.cpu() if _cv._is_torch(T) else T, np.float64)
    except (TypeError, ValueError):
        raise _cv.error(f"{who}: {name} must be a 4 x 4 matrix of numbers") from None
    if M.shape != (4, 4) or not np.isfinite(M).all() or M[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
        raise _cv.error(f"{who}: {name} is not a finite 4 x 4 matrix with the last row (0, 0, 0, 1)")
    return np.ascontiguousarray(M)


def _icp_clouds(who, source, target, source_disparity, target_disparity, target_normals):
    """the two clouds of a registration call, both numpy arrays or both HIP tensors on one GPU, checked:
    (on_device, source, source disparities, target, target disparities, target normals)"""
    on_device = _cv._is_torch(source)
    if on_device != _cv._is_torch(target):
        raise _cv.error(f"{who}: source and target must both be numpy arrays or both be tensors")
    if on_device:
        import torch
        s, ds = _device_cloud(who + " (source)", source, source_disparity, None, 0)
        t, dt = _device_cloud(who + " (target)", target, target_disparity, None, 0)
        if s.device != t.device:
            raise _cv.error(f"{who}: source and target must be on the same GPU")
        nrm = target_normals
        if nrm is not None:
            if not _cv._is_torch(nrm) or nrm.device != t.device or nrm.dtype != torch.float32 or tuple(nrm.shape) != tuple(t.shape):
                raise _cv.error(f"{who}: target_normals must be a float32 tensor of the target's shape on the same GPU")
            nrm = nrm.contiguous()
        ns, nt = s.numel() // 3, t.numel() // 3
    else:
        s, ds, _ = _outlier_cloud(who + " (source)", source, None, source_disparity, None, 0)
        t, dt, _ = _outlier_cloud(who + " (target)", target, None, target_disparity, None, 0)
        nrm = target_normals
        if nrm is not None:
            nrm = np.asarray(nrm)
            if nrm.dtype != np.float32 or nrm.shape != t.shape:
                raise _cv.error(f"{who}: target_normals must be float32 and have the shape of target")
        for name, d in (("source_disparity", ds), ("target_disparity", dt)):
            if d is not None and d.dtype != np.float32:
                raise _cv.error(f"{who}: {name} must be float32 (in pixels), not {d.dtype}")
        ns, nt = s.size // 3, t.size // 3
    if max(ns, nt) > RADIUS_MAX_POINTS:
        raise _cv.error(f"{who}: {max(ns, nt)} points, more than {RADIUS_MAX_POINTS} (include/sgm_hip_icp.h)")
    return on_device, s, ds, t, dt, nrm, ns, nt


def _icp_call(who, source, target, r, T0, estimation, target_normals, source_disparity, target_disparity, max_iteration, rel_f, rel_r,
              origin, evaluate):
    """registration_icp and evaluate_registration behind their argument checks: (T, fitness, rmse, corr, d2, history, stats)"""
    r, org = _search_radius(who, "max_correspondence_distance", r, origin)
    on_device, s, ds, t, dt, nrm, ns, nt = _icp_clouds(who, source, target, source_disparity, target_disparity, target_normals)
    if estimation == 1 and nrm is None:
        raise _cv.error(f"{who}: point_to_plane needs target_normals (estimate_normals_radius on the target)")
    shape = tuple(s.shape[:-1])
    if ns == 0:      # nothing to send to the device
        st = np.zeros(8, np.uint64)
        st[7] = 2
        corr, d2 = np.full(shape, -1, np.int32), np.full(shape, np.nan, np.float32)
        if on_device:
            import torch
            corr, d2 = torch.from_numpy(corr).to(s.device), torch.from_numpy(d2).to(s.device)
        return T0, 0.0, 0.0, corr, d2, np.zeros((1, 2), np.float64), st
    if on_device:
        import torch
        dev = s.device
        corr = torch.full(shape, -1, dtype=torch.int32, device=dev)
        d2 = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
        e = _cv.get_engine(_cv._DEFAULT, dev.index)
        torch.cuda.synchronize(dev)      # the inputs were made on torch's stream, the call runs on the engine's
        ptr = lambda a: None if a is None else a.data_ptr()
        if evaluate:
            fit, rmse, st = e.evaluate_registration_device(s.data_ptr(), ptr(ds), ns, t.data_ptr(), ptr(dt), nt, float(r), org, T0,
                                                           corr.data_ptr(), d2.data_ptr())
            T, hist = T0, np.array([[fit, rmse]], np.float64)
        else:
            T, fit, rmse, hist, st = e.register_icp_device(s.data_ptr(), ptr(ds), ns, t.data_ptr(), ptr(dt), ptr(nrm), nt, float(r), org, T0,
                                                           estimation, max_iteration, rel_f, rel_r, corr.data_ptr(), d2.data_ptr())
        return T, fit, rmse, corr, d2, hist, st
    e = _cv.get_engine(_cv._DEFAULT)
    if evaluate:
        fit, rmse, corr, d2, st = e.evaluate_registration_host(s, ds, t, dt, float(r), org, T0)
        T, hist = T0, np.array([[fit, rmse]], np.float64)
    else:
        T, fit, rmse, corr, d2, hist, st = e.register_icp_host(s, ds, t, dt, nrm, float(r), org, T0, estimation, max_iteration, rel_f, rel_r)
    return T, fit, rmse, corr.reshape(shape), d2.reshape(shape), hist, st


def registration_icp(source, target, max_correspondence_distance, init=None, estimation="point_to_plane", target_normals=None,
                     source_disparity=None, target_disparity=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
                     origin=(0, 0, 0), return_correspondences=False, return_history=False, return_stats=False):
    """Rigid registration of two clouds by iterated closest points, on the GPU: the 4 x 4 transformation that lays `source` on
    `target`, the share of the valid source points that find a target point within max_correspondence_distance (fitness) and the
    root mean square distance of those pairs (inlier_rmse).  Each iteration transforms the source by the current estimate in
    float32, gives every source point its nearest target point within the distance on the target's grid of cells (ties in the float32
    squared distance: the lowest target index), sums the 6 x 6 Gauss-Newton system of the pairs in one fixed pairwise tree in
    float64, solves it on the host by LDL^T and updates the estimate by a quaternion.  estimation: "point_to_plane" (needs
    target_normals; a pair whose normal is not about unit length counts but does not vote) or "point_to_point".  It stops when
    fitness and rmse both change by less than relative_fitness and relative_rmse, after max_iteration (0 .. 1000) iterations, with
    fewer than 6 pairs, or on a system that is not positive definite (a single plane under point_to_plane).
    The definition is include/sgm_hip_icp.h, our own, and the result is the same bits on every run: it is NOT Open3D's
    registration_icp -- the correspondence tie rule; the range rule (target points and transformed source points whose cell index,
    cells of edge max_correspondence_distance * 1.03125 anchored at origin, leaves -2^16 .. 2^16 - 1 take no part); point_to_point
    by the same Gauss-Newton step, not Umeyama's closed form; a quaternion update, not Euler angles; tree-ordered sums; and the two
    thresholds are absolute differences.
    source, target: XYZ images (H, W, 3) with their source_disparity / target_disparity (H, W) -- a point takes part iff X, Y, Z are
    finite and its disparity > 0 -- or (N, 3) lists with no disparity (every finite point takes part); numpy arrays, or HIP tensors
    (float32, on one GPU), which stay on the device.  target_normals: float32 of target's shape.  init: the first estimate (None:
    the identity).
    Returns (transformation float64 (4, 4), fitness, inlier_rmse[, correspondences, distances2][, history][, stats]):
    correspondences int32 of the source's point shape, the target index or -1; distances2 float32, the squared distance or NaN;
    history float64 (evaluations, 2), fitness and rmse of every evaluation from the one under init on; stats a dict: valid_source,
    target_in_range, target_out_of_range, iterations, correspondences, unplaced, unusable_normals, status ("converged",
    "max_iteration", "too_few", "degenerate").

    The chain this exists for -- two clouds merged into one:

        s, _ = voxel_down_sample(source_xyz, None, source_disp, voxel)
        t, _ = voxel_down_sample(target_xyz, None, target_disp, voxel)
        n = estimate_normals_radius(t, None, 2 * voxel)
        T, fitness, rmse = registration_icp(s, t, 2 * voxel, target_normals=n)
        merged = np.concatenate([transform_points(s, T), t])
        write_ply(path, merged)

    In short voxel_down_sample -> estimate_normals_radius (target) -> registration_icp -> transform_points -> concatenate -> write_ply.
    """
    who = "registration_icp"
    if estimation not in ICP_ESTIMATIONS:
        raise _cv.error(f"{who}: estimation={estimation!r} is not one of {ICP_ESTIMATIONS}")
    est = ICP_ESTIMATIONS.index(estimation)
    _int_arg(who, max_iteration, 0, ICP_MAX_ITERATION, f"max_iteration={max_iteration!r} is not an integer in 0 .. {ICP_MAX_ITERATION}")
    rel = []
    for name, v in (("relative_fitness", relative_fitness), ("relative_rmse", relative_rmse)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise _cv.error(f"{who}: {name} must be a number") from None
        if isinstance(v, bool) or not f >= 0:
            raise _cv.error(f"{who}: {name}={v!r} is not a number >= 0")
        rel.append(f)
    T0 = _icp_matrix(who, "init", init)
    T, fit, rmse, corr, d2, hist, st = _icp_call(who, source, target, max_correspondence_distance, T0, est, target_normals, source_disparity,
                                                 target_disparity, int(max_iteration), rel[0], rel[1], origin, False)
    out = (T, fit, rmse)
    if return_correspondences:
        out += (corr, d2)
    if return_history:
        out += (hist,)
    if return_stats:
        d = dict(zip(ICP_STATS, (int(x) for x in st)))
        d["status"] = ICP_STATUS[d["status"]]
        out += (d,)
    return out


def evaluate_registration(source, target, max_correspondence_distance, transformation=None, source_disparity=None, target_disparity=None,
                          origin=(0, 0, 0), return_correspondences=False, return_stats=False):
    """The correspondence pass of registration_icp alone under the caller's transformation (None: the identity), on the GPU: fitness
    and inlier_rmse of include/sgm_hip_icp.h, as registration_icp with max_iteration=0 reports them (NOT Open3D's
    evaluate_registration: the tie rule, the range rule and the tree-ordered sum of that header).  The clouds, origin and the
    optional results are registration_icp's.
    Returns (fitness, inlier_rmse[, correspondences, distances2][, stats])."""
    who = "evaluate_registration"
    T0 = _icp_matrix(who, "transformation", transformation)
    _, fit, rmse, corr, d2, _, st = _icp_call(who, source, target, max_correspondence_distance, T0, 0, None, source_disparity,
                                              target_disparity, 0, 0.0, 0.0, origin, True)
    out = (fit, rmse)
    if return_correspondences:
        out += (corr, d2)
    if return_stats:
        d = dict(zip(ICP_STATS, (int(x) for x in st)))
        d["status"] = ICP_STATUS[d["status"]]
        out += (d,)
    return out


def transform_points(points, transformation, normals=None):
    """The points under a rigid transformation, on the GPU, in the arithmetic registration_icp itself uses (include/sgm_hip_icp.h,
    step 2: the matrix rounded to float32, three fused multiply-adds per coordinate from the translation), so that a registered
    cloud can be merged with its target; normals, if given, by the rotation part only.  points, normals: float32 (..., 3), numpy
    arrays or HIP tensors, which stay on the device; rows that are not finite stay not finite.
    Returns points, or (points, normals) with normals."""
    who = "transform_points"
    T = _icp_matrix(who, "transformation", transformation)
    if transformation is None:
        raise _cv.error(f"{who}: transformation is not a finite 4 x 4 matrix with the last row (0, 0, 0, 1)")
    if _cv._is_torch(points):
        import torch
        p = points
        if not p.is_cuda or p.dtype != torch.float32 or p.dim() < 1 or p.shape[-1] != 3:
            raise _cv.error(f"{who}: a tensor points must be float32 (..., 3) and on the GPU")
        nrm = normals
        if nrm is not None and (not _cv._is_torch(nrm) or nrm.device != p.device or nrm.dtype != torch.float32
                                or tuple(nrm.shape) != tuple(p.shape)):
            raise _cv.error(f"{who}: normals must be a float32 tensor of the points' shape on the same GPU")
        p = p.contiguous()
        nrm = None if nrm is None else nrm.contiguous()
        out, out_n = torch.empty_like(p), None if nrm is None else torch.empty_like(nrm)
        if p.numel():
            e = _cv.get_engine(_cv._DEFAULT, p.device.index)
            torch.cuda.synchronize(p.device)
            e.transform_points_device(p.data_ptr(), None if nrm is None else nrm.data_ptr(), p.numel() // 3, T, out.data_ptr(),
                                      None if out_n is None else out_n.data_ptr())
            e.synchronize()
    else:
        p = np.asarray(points)
        if p.dtype != np.float32 or p.ndim < 1 or p.shape[-1] != 3:
            raise _cv.error(f"{who}: points must be float32 (..., 3), not {p.dtype} {p.shape}")
        nrm = normals
        if nrm is not None:
            nrm = np.asarray(nrm)
            if nrm.dtype != np.float32 or nrm.shape != p.shape:
                raise _cv.error(f"{who}: normals must be float32 and have the shape of points")
        if p.size // 3 > RADIUS_MAX_POINTS:
            raise _cv.error(f"{who}: {p.size // 3} points, more than {RADIUS_MAX_POINTS} (include/sgm_hip_icp.h)")
        if p.size == 0:
            out, out_n = p.copy(), None if nrm is None else nrm.copy()
        else:
            out, out_n = _cv.get_engine(_cv._DEFAULT).transform_points_host(p, T, nrm)
    return out if normals is None else (out, out_n)


MESH_MAX_PIXELS = 1 << 26


def _grid_args(who, points_3D, colors, disparity_map, max_diff, confidence, min_confidence):
    """the argument checks the functions over the organised cloud share, raised before any engine exists: (points, colors,
    disparity with the confidence mask applied, max_diff as float32)"""
    pts = np.asarray(points_3D)
    if pts.dtype != np.float32:
        raise _cv.error(f"{who}: points_3D must be float32, not {pts.dtype}")
    if disparity_map is None:
        raise _cv.error(f"{who}: needs the disparity_map of the points")
    disp = np.asarray(disparity_map)
    if pts.ndim != 3 or pts.shape[2] != 3 or pts.shape[:2] != disp.shape:
        raise _cv.error(f"{who}: points_3D must be (H, W, 3) and disparity_map (H, W)")
    if disp.dtype != np.float32:
        raise _cv.error(f"{who}: disparity_map must be float32 (in pixels), not {disp.dtype}")
    if confidence is not None:
        disp = mask_by_confidence(disp, confidence, min_confidence)
    if colors is not None:
        colors = np.asarray(colors)
        if colors.shape != pts.shape or colors.dtype != np.uint8:
            raise _cv.error(f"{who}: colors must be uint8 and have the shape of points_3D")
    with np.errstate(all="ignore"):
        try:
            md = np.float32(max_diff)
        except (TypeError, ValueError):
            raise _cv.error(f"{who}: max_diff must be a number") from None
    if isinstance(max_diff, bool) or md.shape != () or not np.isfinite(md) or not md >= 0:
        raise _cv.error(f"{who}: max_diff={max_diff!r} is not a finite float32 >= 0")
    H, W = disp.shape
    if H * W > MESH_MAX_PIXELS:
        raise _cv.error(f"{who}: {H} x {W} pixels, more than {MESH_MAX_PIXELS} (include/sgm_hip_mesh.h)")
    return pts, colors, disp, md


def triangulate_points(points_3D, colors, disparity_map, max_diff=1.0, confidence=None, min_confidence=0):
    """A triangle mesh over the organised cloud, on the GPU: two triangles per pixel quad wherever the disparity is continuous --
    a pixel counts iff X, Y, Z are finite and its disparity > 0 (with a confidence map also confidence >= min_confidence, as in
    valid_points), two pixels are connected iff their disparities differ by max_diff at most, each quad is cut along the diagonal
    with the smaller disparity difference, and a triangle is kept iff its three edges are connected.  The vertices are the pixels
    that a triangle uses, in row-major order; the triangles come in row-major order of their quads and face the camera.  The
    definition is include/sgm_hip_mesh.h, our own, and the result is the same bits on every run: it is NOT Open3D's meshing nor
    any other library's.
    points_3D float32 (H, W, 3), disparity_map float32 (H, W) in pixels, colors uint8 (H, W, 3) or None.
    Returns (vertices float32 (V, 3), colors uint8 (V, 3) or None, triangles int32 (F, 3))."""
    pts, colors, disp, md = _grid_args("triangulate_points", points_3D, colors, disparity_map, max_diff, confidence, min_confidence)
    H, W = disp.shape
    if H < 2 or W < 2:     # no quad: nothing to send to the device
        return np.zeros((0, 3), np.float32), None if colors is None else np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32)
    return _cv.get_engine(_cv._DEFAULT).mesh_grid_host(pts, disp, colors, float(md))


def estimate_normals(points_3D, disparity_map, max_diff=1.0, confidence=None, min_confidence=0, orient=True):
    """One unit normal per pixel of the organised cloud, on the GPU: the sum of the (area-weighted) normals of the triangles of
    triangulate_points around the pixel -- same validity, same max_diff, same confidence mask --, normalised, and with orient
    turned so that it points towards the camera at the origin.  Pixels that no triangle uses get (0, 0, 0).  The definition is
    include/sgm_hip_normals.h, our own, every operation and its order written out, and the result is the same bits on every run:
    it is NOT Open3D's estimate_normals (no neighbour search, no covariance) nor any other library's.
    points_3D float32 (H, W, 3), disparity_map float32 (H, W) in pixels.  Returns float32 (H, W, 3)."""
    pts, _, disp, md = _grid_args("estimate_normals", points_3D, None, disparity_map, max_diff, confidence, min_confidence)
    if disp.shape[0] < 2 or disp.shape[1] < 2:     # no quad, no vertex: nothing to send to the device
        return np.zeros(disp.shape + (3,), np.float32)
    return _cv.get_engine(_cv._DEFAULT).normals_grid_host(pts, disp, float(md), bool(orient))


def triangulate_points_with_normals(points_3D, colors, disparity_map, max_diff=1.0, confidence=None, min_confidence=0, orient=True):
    """triangulate_points and one unit normal per vertex: the rows of estimate_normals at the vertices' pixels, computed in the same
    call.  The faces keep their winding whatever orient turns.  The definition is include/sgm_hip_normals.h, our own: it is NOT
    Open3D's compute_vertex_normals nor any other library's.
    Returns (vertices float32 (V, 3), colors uint8 (V, 3) or None, triangles int32 (F, 3), normals float32 (V, 3))."""
    pts, colors, disp, md = _grid_args("triangulate_points_with_normals", points_3D, colors, disparity_map, max_diff, confidence,
                                       min_confidence)
    if disp.shape[0] < 2 or disp.shape[1] < 2:     # no quad: nothing to send to the device
        return (np.zeros((0, 3), np.float32), None if colors is None else np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32),
                np.zeros((0, 3), np.float32))
    return _cv.get_engine(_cv._DEFAULT).mesh_grid_normals_host(pts, disp, colors, float(md), bool(orient))


def write_triangle_mesh(filename, vertices, triangles, colors=None, binary=True) -> bool:
    """PLY export of a triangle mesh (triangulate_points) in the layout Open3D writes for one: vertices double x/y/z, uchar
    red/green/blue when colours are given, then `element face F` with `property list uchar uint vertex_indices`.  Triangles that
    index outside the vertex list are refused."""
    pts = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    tri = np.asarray(triangles)
    if tri.dtype.kind not in "iu" or tri.ndim != 2 or tri.shape[1] != 3:
        raise _cv.error("write_triangle_mesh: triangles must be an integer (F, 3) array")
    if tri.size and (int(tri.min()) < 0 or int(tri.max()) >= n):
        raise _cv.error(f"write_triangle_mesh: a triangle indexes outside the {n} vertices")
    nf = tri.shape[0]
    if colors is not None:
        col = np.asarray(colors)
        if col.dtype != np.uint8 or col.shape != (n, 3):
            raise _cv.error("write_triangle_mesh: colors must be uint8 and one row per vertex")
    else:
        col = None
    head = ["ply", "format binary_little_endian 1.0" if binary else "format ascii 1.0",
            "comment stereo_reconstruction_cv_amd", f"element vertex {n}",
            "property double x", "property double y", "property double z"]
    if col is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += [f"element face {nf}", "property list uchar uint vertex_indices", "end_header"]
    with open(filename, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            if col is None:
                pts.astype("<f8").tofile(f)
            else:
                rec = np.empty(n, dtype=[("p", "<f8", 3), ("c", "u1", 3)])
                rec["p"], rec["c"] = pts, col
                rec.tofile(f)
            frec = np.empty(nf, dtype=[("k", "u1"), ("v", "<u4", 3)])
            frec["k"], frec["v"] = 3, tri
            frec.tofile(f)
        else:
            for i in range(n):
                line = " ".join(repr(float(v)) for v in pts[i])
                if col is not None:
                    line += " " + " ".join(str(int(v)) for v in col[i])
                f.write((line + "\n").encode("ascii"))
            for t in tri:
                f.write(("3 " + " ".join(str(int(v)) for v in t) + "\n").encode("ascii"))
    return True


def read_triangle_mesh(filename):
    """Minimal reader for files written by write_triangle_mesh (used by the tests): (vertices float64 (V, 3), colors uint8 (V, 3)
    or None, triangles int32 (F, 3))."""
    with open(filename, "rb") as f:
        header = []
        while True:
            line = f.readline().decode("ascii").strip()
            header.append(line)
            if line == "end_header":
                break
        n = int([h for h in header if h.startswith("element vertex")][0].split()[-1])
        nf = int([h for h in header if h.startswith("element face")][0].split()[-1])
        if "property list uchar uint vertex_indices" not in header:
            raise _cv.error("read_triangle_mesh: not a face list of uchar counts and uint indices")
        has_col = any(h.endswith(" red") for h in header)
        if "format binary_little_endian 1.0" in header:
            dt = [("p", "<f8", 3)] + ([("c", "u1", 3)] if has_col else [])
            rec = np.fromfile(f, dtype=dt, count=n)
            frec = np.fromfile(f, dtype=[("k", "u1"), ("v", "<u4", 3)], count=nf)
            if rec.shape[0] != n or frec.shape[0] != nf or (frec["k"] != 3).any():
                raise _cv.error("read_triangle_mesh: the file is cut short or a face is no triangle")
            return rec["p"].copy(), (rec["c"].copy() if has_col else None), frec["v"].astype(np.int32)
        rows = [f.readline().decode("ascii").split() for _ in range(n)]
        pts = np.array([[float(v) for v in r[:3]] for r in rows], np.float64).reshape(n, 3)
        col = np.array([[int(v) for v in r[3:6]] for r in rows], np.uint8).reshape(n, 3) if has_col else None
        frows = [f.readline().decode("ascii").split() for _ in range(nf)]
        if any(len(r) != 4 or r[0] != "3" for r in frows):
            raise _cv.error("read_triangle_mesh: the file is cut short or a face is no triangle")
        return pts, col, np.array([[int(v) for v in r[1:]] for r in frows], np.int32).reshape(nf, 3)


def write_point_cloud(filename, points, colors=None, binary=True) -> bool:
    """PLY export of a point list; `points` (N,3) or (H,W,3), non-finite points are written as they
    are (the notebook saves the unmasked H*W points, main.ipynb:795-797).  Same property layout
    as Open3D's writer: double x/y/z, uchar red/green/blue when colours are given."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    if colors is not None:
        col = np.asarray(colors).reshape(-1, 3)
        if col.shape[0] != n:
            raise _cv.error("write_point_cloud: colors and points differ in length")
        if col.dtype != np.uint8:  # Open3D keeps colours in [0,1]; accept both
            col = np.clip(np.rint(np.asarray(col, np.float64) * (255.0 if col.max(initial=0) <= 1.0 else 1.0)), 0, 255).astype(np.uint8)
    else:
        col = None
    head = ["ply", "format binary_little_endian 1.0" if binary else "format ascii 1.0",
            "comment stereo_reconstruction_cv_amd", f"element vertex {n}",
            "property double x", "property double y", "property double z"]
    if col is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head.append("end_header")
    with open(filename, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            if col is None:
                pts.astype("<f8").tofile(f)
            else:
                rec = np.empty(n, dtype=[("p", "<f8", 3), ("c", "u1", 3)])
                rec["p"], rec["c"] = pts, col
                rec.tofile(f)
        else:
            for i in range(n):
                line = " ".join(repr(float(v)) for v in pts[i])
                if col is not None:
                    line += " " + " ".join(str(int(v)) for v in col[i])
                f.write((line + "\n").encode("ascii"))
    return True


def read_point_cloud(filename):
    """Minimal reader for files written by write_point_cloud (used by the tests)."""
    with open(filename, "rb") as f:
        header = []
        while True:
            line = f.readline().decode("ascii").strip()
            header.append(line)
            if line == "end_header":
                break
        n = int([h for h in header if h.startswith("element vertex")][0].split()[-1])
        has_col = any("red" in h for h in header)
        if "format binary_little_endian 1.0" in header:
            dt = [("p", "<f8", 3)] + ([("c", "u1", 3)] if has_col else [])
            rec = np.fromfile(f, dtype=dt, count=n)
            return rec["p"].copy(), (rec["c"].copy() if has_col else None)
        rows = [f.readline().decode("ascii").split() for _ in range(n)]
        pts = np.array([[float(v) for v in r[:3]] for r in rows], np.float64).reshape(n, 3)
        col = np.array([[int(v) for v in r[3:6]] for r in rows], np.uint8).reshape(n, 3) if has_col else None
        return pts, col


def write_ply(filename, points, colors=None, normals=None, triangles=None, binary=True) -> bool:
    """One PLY writer for a cloud or a mesh, with or without normals and colours: vertex properties double x/y/z, then double
    nx/ny/nz, then uchar red/green/blue, then with triangles the face list of write_triangle_mesh -- the order Open3D writes.
    Without normals the file equals write_point_cloud's (triangles None) or write_triangle_mesh's byte for byte."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    cols = [("p", pts)]
    if normals is not None:
        nrm = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
        if nrm.shape[0] != n:
            raise _cv.error("write_ply: normals and points differ in length")
        cols.append(("n", nrm))
    if colors is not None:
        col = np.asarray(colors).reshape(-1, 3)
        if col.shape[0] != n:
            raise _cv.error("write_ply: colors and points differ in length")
        if col.dtype != np.uint8:  # as write_point_cloud: colours in [0, 1] or [0, 255]
            col = np.clip(np.rint(np.asarray(col, np.float64) * (255.0 if col.max(initial=0) <= 1.0 else 1.0)), 0, 255).astype(np.uint8)
        cols.append(("c", col))
    tri = None
    if triangles is not None:
        tri = np.asarray(triangles)
        if tri.dtype.kind not in "iu" or tri.ndim != 2 or tri.shape[1] != 3:
            raise _cv.error("write_ply: triangles must be an integer (F, 3) array")
        if tri.size and (int(tri.min()) < 0 or int(tri.max()) >= n):
            raise _cv.error(f"write_ply: a triangle indexes outside the {n} vertices")
    names = dict(p=["double x", "double y", "double z"], n=["double nx", "double ny", "double nz"],
                 c=["uchar red", "uchar green", "uchar blue"])
    head = ["ply", "format binary_little_endian 1.0" if binary else "format ascii 1.0",
            "comment stereo_reconstruction_cv_amd", f"element vertex {n}"]
    head += ["property " + prop for k, _ in cols for prop in names[k]]
    if tri is not None:
        head += [f"element face {tri.shape[0]}", "property list uchar uint vertex_indices"]
    head.append("end_header")
    with open(filename, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            rec = np.empty(n, dtype=[(k, "u1" if k == "c" else "<f8", 3) for k, _ in cols])
            for k, a in cols:
                rec[k] = a
            rec.tofile(f)
            if tri is not None:
                frec = np.empty(tri.shape[0], dtype=[("k", "u1"), ("v", "<u4", 3)])
                frec["k"], frec["v"] = 3, tri
                frec.tofile(f)
        else:
            for i in range(n):
                line = " ".join(" ".join(str(int(v)) if k == "c" else repr(float(v)) for v in a[i]) for k, a in cols)
                f.write((line + "\n").encode("ascii"))
            for t in (tri if tri is not None else ()):
                f.write(("3 " + " ".join(str(int(v)) for v in t) + "\n").encode("ascii"))
    return True


def read_ply(filename):
    """Minimal reader for files written by write_ply, write_point_cloud and write_triangle_mesh (used by the tests): (points
    float64 (N, 3), colors uint8 (N, 3) or None, normals float64 (N, 3) or None, triangles int32 (F, 3) or None)."""
    with open(filename, "rb") as f:
        header = []
        while True:
            line = f.readline().decode("ascii").strip()
            header.append(line)
            if line == "end_header":
                break
        n = int([h for h in header if h.startswith("element vertex")][0].split()[-1])
        face = [h for h in header if h.startswith("element face")]
        nf = int(face[0].split()[-1]) if face else None
        if face and "property list uchar uint vertex_indices" not in header:
            raise _cv.error("read_ply: not a face list of uchar counts and uint indices")
        has_nrm, has_col = "property double nx" in header, "property uchar red" in header
        if "format binary_little_endian 1.0" in header:
            dt = [("p", "<f8", 3)] + ([("n", "<f8", 3)] if has_nrm else []) + ([("c", "u1", 3)] if has_col else [])
            rec = np.fromfile(f, dtype=dt, count=n)
            tri = None
            if face:
                frec = np.fromfile(f, dtype=[("k", "u1"), ("v", "<u4", 3)], count=nf)
                if frec.shape[0] != nf or (frec["k"] != 3).any():
                    raise _cv.error("read_ply: the file is cut short or a face is no triangle")
                tri = frec["v"].astype(np.int32)
            if rec.shape[0] != n:
                raise _cv.error("read_ply: the file is cut short")
            return rec["p"].copy(), (rec["c"].copy() if has_col else None), (rec["n"].copy() if has_nrm else None), tri
        rows = [f.readline().decode("ascii").split() for _ in range(n)]
        k = 6 if has_nrm else 3
        if any(len(r) != k + 3 * has_col for r in rows):
            raise _cv.error("read_ply: the file is cut short")
        pts = np.array([[float(v) for v in r[:3]] for r in rows], np.float64).reshape(n, 3)
        nrm = np.array([[float(v) for v in r[3:6]] for r in rows], np.float64).reshape(n, 3) if has_nrm else None
        col = np.array([[int(v) for v in r[k:k + 3]] for r in rows], np.uint8).reshape(n, 3) if has_col else None
        tri = None
        if face:
            frows = [f.readline().decode("ascii").split() for _ in range(nf)]
            if any(len(r) != 4 or r[0] != "3" for r in frows):
                raise _cv.error("read_ply: the file is cut short or a face is no triangle")
            tri = np.array([[int(v) for v in r[1:]] for r in frows], np.int32).reshape(nf, 3)
        return pts, col, nrm, tri


# ---- many frames fused into one model: the truncated signed distance volume (include/sgm_hip_tsdf.h) ------------------------------
TSDF_STATS = ("updated", "unclamped", "no_depth", "occluded", "saturated", "outside", "usable_pixels")
TSDF_MAX_DIM = 4096
TSDF_MAX_VOXELS = 1 << 30
TSDF_MAX_PIXELS = 1 << 27
TSDF_MAX_WEIGHT = 65535


def camera_from_Q(Q):
    """The pinhole camera behind a reprojection matrix Q (cv2.stereoRectify's, the notebook's, synth.default_Q):
    ((fx, fy, cx, cy), front) with fx = fy = Q[2, 3], cx = -Q[0, 3], cy = -Q[1, 3] and front = sign(Q[2, 3] * Q[3, 2]), the sign of
    Z in front of the camera under reprojectImageTo3D with that Q (the notebook's Q gives -1).  Raises unless Q[0, 0] = Q[1, 1] = 1."""
    try:
        Q = np.asarray(Q.cpu() if _cv._is_torch(Q) else Q, np.float64)
    except (TypeError, ValueError):
        raise _cv.error("camera_from_Q: Q must be a 4 x 4 matrix of numbers") from None
    if Q.shape != (4, 4) or not np.isfinite(Q).all():
        raise _cv.error("camera_from_Q: Q must be a finite 4 x 4 matrix")
    if Q[0, 0] != 1.0 or Q[1, 1] != 1.0:
        raise _cv.error("camera_from_Q: Q[0, 0] and Q[1, 1] must be 1 (a Q of another scale is not a pinhole camera in pixels)")
    s = Q[2, 3] * Q[3, 2]
    if s == 0.0:
        raise _cv.error("camera_from_Q: Q[2, 3] * Q[3, 2] is 0: no focal length or no baseline")
    f = float(Q[2, 3])
    return (f, f, float(-Q[0, 3]), float(-Q[1, 3])), (1 if s > 0 else -1)


def invert_rigid(T):
    """The inverse of a rigid transformation in float64: [R | t]^-1 = [R^T | -R^T t].  registration_icp(frame_k, frame_0)
    gives camera k -> world (frame 0); TSDFVolume.integrate wants world -> camera: extrinsic = invert_rigid(T)."""
    if T is None:
        raise _cv.error("invert_rigid: T is None: a rigid transformation (4 x 4) is needed")
    M = _icp_matrix("invert_rigid", "T", T)
    out = np.eye(4, dtype=np.float64)
    out[:3, :3] = M[:3, :3].T
    out[:3, 3] = -(M[:3, :3].T @ M[:3, 3])
    return out


def _tsdf_positive(who, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise _cv.error(f"{who}: {name} must be a number")
    f = np.float32(v)
    if not np.isfinite(f) or not f > 0:
        raise _cv.error(f"{who}: {name} must be finite and positive in float32, not {v!r}")
    return float(f)


class TSDFVolume:
    """A dense truncated signed distance volume that fuses many frames into one denoised surface, on the GPU
    (include/sgm_hip_tsdf.h).  It stands where Open3D's UniformTSDFVolume / ScalableTSDFVolume stand in user code, but it is NOT
    Open3D's integration: the depth is the Z of the XYZ image, the distance is taken along the camera's Z axis and quantised to
    1 / 32767 of sdf_trunc, each voxel keeps an INTEGER sum and count (so the order of the frames does not matter, up to 65535
    frames per voxel), and the extraction interpolates the zero crossing on every voxel edge in index order.

    TSDFVolume(voxel_size, sdf_trunc, dims=(nx, ny, nz), origin=(0, 0, 0), color=True, device=None): the voxel (i, j, k) has its
    centre at origin + (i + .5, j + .5, k + .5) * voxel_size, in the world frame.  The planes .sum, .weight (int32 (nz, ny, nx))
    and .rgb_sum (uint32 (3, nz, ny, nx), None without color) are HIP tensors when `device` (a GPU index or True; the default
    wherever a GPU is present), else numpy arrays; reset() zeroes them.

    The chain, per frame k:  compute -> reprojectImageTo3D -> registration_icp(frame k, frame 0) -> vol.integrate(points_3D, colors,
    disparity_map, camera_from_Q(Q)[0], extrinsic=invert_rigid(T));  once:  extract_point_cloud -> estimate_normals_radius ->
    write_ply.
    Not offered: a hashed or sparse volume, truncation scaled with depth, weights other than 1, normals from the gradient, a
    marching-cubes mesh, ray casting, a batch of frames per call."""

    def __init__(self, voxel_size, sdf_trunc, dims, origin=(0, 0, 0), color=True, device=None):
        who = "TSDFVolume"
        self.voxel_size = _tsdf_positive(who, "voxel_size", voxel_size)
        self.sdf_trunc = _tsdf_positive(who, "sdf_trunc", sdf_trunc)
        with np.errstate(all="ignore"):
            kappa = np.float32(32767.0) / np.float32(self.sdf_trunc)
        if not np.isfinite(kappa):
            raise _cv.error(f"{who}: 32767 / sdf_trunc is not finite in float32")
        try:
            d = [v for v in dims]
        except TypeError:
            d = []
        if len(d) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= TSDF_MAX_DIM for v in d):
            raise _cv.error(f"{who}: dims must be three integers (nx, ny, nz) in 1 .. {TSDF_MAX_DIM}")
        self.dims = tuple(int(v) for v in d)
        nx, ny, nz = self.dims
        if nx * ny * nz > TSDF_MAX_VOXELS:
            raise _cv.error(f"{who}: {nx * ny * nz} voxels, more than 2^30")
        try:
            org = np.asarray(origin, np.float32).reshape(-1)
        except (TypeError, ValueError):
            org = np.zeros(0, np.float32)
        if org.shape != (3,) or not np.isfinite(org).all():
            raise _cv.error(f"{who}: origin must be three finite numbers")
        self.origin = tuple(float(v) for v in org)
        self.color = bool(color)
        if device is None:      # the GPU wherever there is one; a library that does not load is an error, not a reason for numpy planes
            device = _cv.get_device() if _cv._lib.load().sgm_device_count() > 0 else False
        if device is True:
            device = _cv.get_device()
        self.device = None if device is False else int(device)
        if self.device is None:
            self.sum, self.weight = np.zeros((nz, ny, nx), np.int32), np.zeros((nz, ny, nx), np.int32)
            self.rgb_sum = np.zeros((3, nz, ny, nx), np.uint32) if self.color else None
        else:
            import torch
            dev = torch.device("cuda", self.device)
            self.sum, self.weight = torch.zeros((nz, ny, nx), dtype=torch.int32, device=dev), torch.zeros((nz, ny, nx), dtype=torch.int32, device=dev)
            # (torch has no uint32 arithmetic worth the name: the bytes are uint32, the tensor's dtype is int32)
            self.rgb_sum = torch.zeros((3, nz, ny, nx), dtype=torch.int32, device=dev) if self.color else None

    def reset(self):
        """The empty volume: every plane zero."""
        for p in (self.sum, self.weight, self.rgb_sum):
            if p is not None:
                p.fill_(0) if _cv._is_torch(p) else p.fill(0)

    def _engine(self):
        return _cv.get_engine(_cv._DEFAULT, self.device)

    def integrate(self, points_3D, colors, disparity_map, intrinsic, extrinsic=None, front=None, max_depth=None, confidence=None,
                  min_confidence=0, return_stats=False):
        """One frame into the volume.  points_3D float32 (H, W, 3) -- reprojectImageTo3D's image --, colors uint8 (H, W, 3) (needed
        iff the volume has colour; ignored otherwise), disparity_map float32 (H, W) or None: arrays or HIP tensors.  intrinsic:
        (fx, fy, cx, cy) in pixels (camera_from_Q(Q)[0]).  extrinsic: world -> camera, 4 x 4 (None: the identity; invert_rigid of an
        ICP result).  front: +1 or -1, the sign of Z in front of the camera; None takes the sign of the median Z of the valid
        pixels.  max_depth: pixels farther than this (|Z|) are not used; None: no limit.  confidence masks the disparity as in every
        other cloud call.  Returns None, or with return_stats the dict of TSDF_STATS."""
        who = "TSDFVolume.integrate"
        on_dev = _cv._is_torch(points_3D)
        if disparity_map is None:
            if confidence is not None:
                raise _cv.error(f"{who}: a confidence map needs a disparity_map")
            if on_dev:
                import torch
                if not points_3D.is_cuda or points_3D.dtype != torch.float32:
                    raise _cv.error(f"{who}: a tensor points_3D must be float32 and on the GPU")
                pts, disp = points_3D.contiguous(), None
            else:
                pts, disp = np.asarray(points_3D), None
                if pts.dtype != np.float32:
                    raise _cv.error(f"{who}: points_3D must be float32, not {pts.dtype}")
            if pts.ndim != 3 or pts.shape[2] != 3:
                raise _cv.error(f"{who}: points_3D must be (H, W, 3)")
        elif on_dev:
            pts, disp = _device_cloud(who, points_3D, disparity_map, confidence, min_confidence)
        else:
            pts, disp, _ = _outlier_cloud(who, points_3D, None, disparity_map, confidence, min_confidence)
            if disp.dtype != np.float32:
                raise _cv.error(f"{who}: disparity_map must be float32, not {disp.dtype}")
        H, W = int(pts.shape[0]), int(pts.shape[1])
        if H < 1 or W < 1 or H * W > TSDF_MAX_PIXELS:
            raise _cv.error(f"{who}: a frame of {H} x {W} pixels (1 .. 2^27 are supported)")
        col = None
        if self.color:
            if colors is None:
                raise _cv.error(f"{who}: the volume has colour: colors must be uint8 (H, W, 3)")
            if _cv._is_torch(colors):
                import torch
                if colors.dtype != torch.uint8 or tuple(colors.shape) != (H, W, 3):
                    raise _cv.error(f"{who}: colors must be uint8 and have the shape of points_3D")
                col = colors
            else:
                col = np.asarray(colors)
                if col.dtype != np.uint8 or col.shape != (H, W, 3):
                    raise _cv.error(f"{who}: colors must be uint8 and have the shape of points_3D")
        try:
            cam = np.asarray(intrinsic, np.float32).reshape(-1)
        except (TypeError, ValueError):
            cam = np.zeros(0, np.float32)
        if cam.shape != (4,) or not np.isfinite(cam).all():
            raise _cv.error(f"{who}: intrinsic must be four finite numbers (fx, fy, cx, cy)")
        T = _icp_matrix(who, "extrinsic", extrinsic)
        if max_depth is None:
            max_depth = float("inf")
        elif isinstance(max_depth, bool) or not isinstance(max_depth, (int, float, np.integer, np.floating)) or not np.float32(max_depth) > 0:
            raise _cv.error(f"{who}: max_depth must be a number > 0 or None")
        if front is None:
            if on_dev:
                import torch
                ok = torch.isfinite(pts).all(dim=2) if disp is None else torch.isfinite(pts).all(dim=2) & (disp > 0)
                z = pts[..., 2][ok]
                front = -1 if z.numel() and float(z.median()) < 0 else 1
            else:
                ok = np.isfinite(pts).all(axis=2) if disp is None else np.isfinite(pts).all(axis=2) & (disp > 0)
                z = pts[..., 2][ok]
                front = -1 if z.size and float(np.median(z)) < 0 else 1
        elif isinstance(front, bool) or front not in (1, -1):
            raise _cv.error(f"{who}: front must be +1, -1 or None")
        front = int(front)
        e = self._engine()
        if self.device is None:
            to_np = lambda a: None if a is None else (a.cpu().numpy() if _cv._is_torch(a) else a)
            st = e.tsdf_integrate_host(self.dims, self.voxel_size, self.sdf_trunc, self.origin, self.sum, self.weight, self.rgb_sum,
                                       to_np(pts), to_np(disp), to_np(col), cam, front, T, max_depth, stats=return_stats)
        else:
            import torch
            dev = self.sum.device
            to_t = lambda a: None if a is None else (a.to(dev) if _cv._is_torch(a) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)).contiguous()
            pts, disp, col = to_t(pts), to_t(disp), to_t(col)
            ptr = lambda a: None if a is None else a.data_ptr()
            torch.cuda.synchronize(dev)
            st = e.tsdf_integrate_device(self.dims, self.voxel_size, self.sdf_trunc, self.origin, self.sum.data_ptr(), self.weight.data_ptr(),
                                         ptr(self.rgb_sum), pts.data_ptr(), ptr(disp), ptr(col), H, W, cam, front, T, max_depth,
                                         stats=return_stats)
            e.synchronize()
        return dict(zip(TSDF_STATS, (int(v) for v in st[:7]))) if return_stats else None

    def extract_point_cloud(self, min_weight=1):
        """The zero crossings of the averaged distance on the voxel edges between voxels that at least min_weight frames saw:
        (points float32 (N, 3), colors uint8 (N, 3) or None), in voxel order, x, y, z edge of a voxel in that order; arrays or HIP
        tensors as the planes are.  Counts first, then allocates."""
        who = "TSDFVolume.extract_point_cloud"
        _int_arg(who, min_weight, 1, (1 << 31) - 1, "min_weight must be an integer >= 1")
        e = self._engine()
        if self.device is None:
            n = e.tsdf_extract_host(self.dims, self.voxel_size, self.origin, self.sum, self.weight, None, min_weight)
            pts = np.empty((n, 3), np.float32)
            col = np.empty((n, 3), np.uint8) if self.color else None
            if n:
                e.tsdf_extract_host(self.dims, self.voxel_size, self.origin, self.sum, self.weight, self.rgb_sum, min_weight, pts, col)
            return pts, col
        import torch
        dev = self.sum.device
        torch.cuda.synchronize(dev)
        rgb = None if self.rgb_sum is None else self.rgb_sum.data_ptr()
        n = e.tsdf_extract_device(self.dims, self.voxel_size, self.origin, self.sum.data_ptr(), self.weight.data_ptr(), None, min_weight)
        pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
        col = torch.empty((n, 3), dtype=torch.uint8, device=dev) if self.color else None
        if n:
            torch.cuda.synchronize(dev)
            e.tsdf_extract_device(self.dims, self.voxel_size, self.origin, self.sum.data_ptr(), self.weight.data_ptr(), rgb, min_weight, n,
                                  pts.data_ptr(), None if col is None else col.data_ptr())
        return pts, col
