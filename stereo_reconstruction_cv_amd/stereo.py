"""Host-side mirror of the cv2 calls on the reference's "Run Disparity" path.

    cv2.StereoSGBM_create(...)            /root/reference/main.ipynb:655-666  -> StereoSGBM_create
    stereo.compute(imgL, imgR)            /root/reference/main.ipynb:668      -> StereoSGBM.compute
    cv2.reprojectImageTo3D(disp, Q)       /root/reference/main.ipynb:697      -> reprojectImageTo3D

Same names, keyword arguments, dtypes and error behaviour (a Python exception, so the
`try/except Exception` of main.ipynb:696-701 still works), routed through the C ABI of
include/sgm_hip.h into hand-written HIP for gfx950.  numpy arrays go through the host-pointer
entry points (blocking, like cv2); torch CUDA tensors go through the device-pointer entry
points and come back as torch tensors on the same device, without touching the host.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import weakref

import numpy as np

from . import _lib

STEREO_SGBM_MODE_SGBM = 0
STEREO_SGBM_MODE_HH = 1
STEREO_SGBM_MODE_SGBM_3WAY = 2
STEREO_SGBM_MODE_HH4 = 3
# the matching cost (setCostFunction; no counterpart in cv2): OpenCV's prefilter + Birchfield-Tomasi, or the 9 x 7 census
# transform with Hamming distance -- exactly invariant under strictly increasing intensity changes of either image
STEREO_COST_BT = _lib.SGM_COST_BT
STEREO_COST_CENSUS = _lib.SGM_COST_CENSUS
CV_32F = 5


class error(Exception):
    """Counterpart of cv2.error."""


_PARAM_NAMES = ("minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff",
                "preFilterCap", "uniquenessRatio", "speckleWindowSize", "speckleRange", "mode")

_DEFAULT = dict(minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0,
                uniquenessRatio=0, speckleWindowSize=0, speckleRange=0, mode=0)

_device = None


def set_device(index: int) -> None:
    """Select the GPU used by engines created afterwards (default: $LOCAL_RANK or 0)."""
    global _device
    _device = int(index)


def get_device() -> int:
    if _device is not None:
        return _device
    return int(os.environ.get("SGM_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def _check(rc: int) -> None:
    if rc != 0:
        raise error(f"sgm_hip error {rc}: {_lib.last_error()}")


def _at(a):
    """The address of an array for a C entry; None (a null pointer) for None."""
    return None if a is None else a.ctypes.data


def _vec3(v) -> np.ndarray:
    return np.ascontiguousarray(v, np.float32).reshape(3)


def _cloud_in(xyz, disp, colors):
    """A point list as the C entries read it: (xyz float32 (n, 3), n, disp float32 (n) or None, colors uint8 (n, 3) or None)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    disp = None if disp is None else np.ascontiguousarray(disp, np.float32).reshape(-1)
    colors = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    return xyz, xyz.shape[0], disp, colors


class Engine:
    """Owns one sgm_engine handle (device buffers + stream) for a fixed parameter set."""

    def __init__(self, params: dict, device: int | None = None, stream: int | None = None):
        self._L = _lib.load()
        params = {**_DEFAULT, **params}     # cv2.StereoSGBM_create defaults for missing keys
        unknown = set(params) - set(_PARAM_NAMES)
        if unknown:
            raise TypeError(f"unknown StereoSGBM parameter(s): {sorted(unknown)}")
        self.params = dict(params)
        self.device = get_device() if device is None else int(device)
        p = _lib.SgmParams(*[int(params[n]) for n in _PARAM_NAMES])
        self._p = p
        h = C.c_void_p()
        _check(self._L.sgm_create(C.byref(p), self.device, C.c_void_p(stream or 0), C.byref(h)))
        self._h = h
        self._fin = weakref.finalize(self, self._L.sgm_destroy, h)
        self._cn = 1                        # SGM_OPT_CHANNELS the engine is set to

    # -- options / introspection
    def set_option(self, opt: int, value: int) -> None:
        _check(self._L.sgm_set_option(self._h, opt, int(value)))
        if opt == _lib.SGM_OPT_CHANNELS:
            self._cn = int(value)

    def _channels(self, cn: int) -> None:
        """Images of the next call have cn interleaved channels (1 or 3); the option is set only when it changes."""
        if cn != self._cn:
            self.set_option(_lib.SGM_OPT_CHANNELS, cn)

    def geometry(self, W: int):
        a, b = C.c_int(), C.c_int()
        _check(self._L.sgm_geometry(C.byref(self._p), W, C.byref(a), C.byref(b)))
        return a.value, b.value

    def algorithmic_bytes(self, H: int, W: int, with_reproject: bool = False) -> int:
        return int(self._L.sgm_algorithmic_bytes(C.byref(self._p), H, W, int(with_reproject)))

    def synchronize(self) -> None:
        _check(self._L.sgm_synchronize(self._h))

    def check(self) -> None:
        """Status WITHOUT waiting for the engine's stream (sgm_check): raises if a chained sweep gave up since the last
        check -- for callers that order the engine's stream with events of their own."""
        _check(self._L.sgm_check(self._h))

    def trim(self) -> None:
        """Give back the internal engines (and their device memory) the batch entries created (sgm_trim)."""
        _check(self._L.sgm_trim(self._h))

    def stage_times(self):
        st = _lib.SgmStageTimes()
        _check(self._L.sgm_get_stage_times(self._h, C.byref(st)))
        return [(st.name[i].decode(), float(st.ms[i]), int(st.launches[i])) for i in range(st.n)]

    def headroom(self) -> dict:
        """Regime record of the last compute (sgm_get_headroom): inside the int16 no-overflow regime
        of OpenCV's StereoSGBM (where this engine's output is bit-exact) iff `ok`."""
        a, b, ok = C.c_int(), C.c_int(), C.c_int()
        _check(self._L.sgm_get_headroom(self._h, C.byref(a), C.byref(b), C.byref(ok)))
        return dict(ok=bool(ok.value), max_cost_plus_p2=a.value, max_delta=b.value)

    def tap(self, which: int, H: int, W: int) -> np.ndarray:
        if which in (_lib.SGM_TAP_COST, _lib.SGM_TAP_AGGR):
            _, W1 = self.geometry(W)
            out = np.empty((H, max(W1, 0), self.params["numDisparities"]), np.int16)
        elif which in (_lib.SGM_TAP_RIGHT_RAW, _lib.SGM_TAP_RIGHT):   # needs SGM_OPT_RIGHT_VIEW = 1 before the compute
            out = np.empty((H, W), np.int16)
        elif which in (_lib.SGM_TAP_CONF_RAW, _lib.SGM_TAP_CONF):     # needs SGM_OPT_CONFIDENCE = 1 before the compute
            out = np.empty((H, W), np.uint8)
        else:
            out = np.empty((H, W), np.int16)
        _check(self._L.sgm_get_tap(self._h, which, out.ctypes.data, out.nbytes))
        return out

    # -- host-pointer path
    def compute_host(self, left: np.ndarray, right: np.ndarray) -> np.ndarray:
        """(H, W) or (H, W, 3) uint8 pair: rows may be padded, pixels must be dense (strides[-1] == 1, and 3 for a
        colour pixel)."""
        H, W = left.shape[:2]
        cn = 1 if left.ndim == 2 else left.shape[2]
        disp = np.empty((H, W), np.int16)
        if left.strides[0] != right.strides[0]:
            right = np.ascontiguousarray(right)
            left = np.ascontiguousarray(left)
        self._channels(cn)
        _check(self._L.sgm_compute(self._h, left.ctypes.data, right.ctypes.data, H, W, left.strides[0],
                                   disp.ctypes.data))
        return disp

    def compute_batch_host(self, lefts: np.ndarray, rights: np.ndarray, Q: np.ndarray | None = None, out=None):
        """N pairs from / to host arrays (sgm_compute_batch).  out: optional (disps int16 [N, H, W][, xyz float32 [N, H, W, 3]])
        arrays to fill -- like the `disparity` argument of cv2's compute(); a caller that runs batch after batch saves the
        page faults of a fresh 17 MB per 4K map (about a millisecond per pair)."""
        N, H, W = lefts.shape[:3]
        cn = 1 if lefts.ndim == 3 else lefts.shape[3]     # (N, H, W) or (N, H, W, 3)
        lefts = np.ascontiguousarray(lefts, np.uint8)
        rights = np.ascontiguousarray(rights, np.uint8)
        if rights.shape != lefts.shape:
            raise error("compute_batch_host: lefts and rights must have the same shape")
        disps = xyz = None
        if out is not None:
            disps, xyz = (out if isinstance(out, (tuple, list)) else (out, None))
            if disps.shape != (N, H, W) or disps.dtype != np.int16 or not disps.flags.c_contiguous:
                raise error("compute_batch_host: out[0] must be a C-contiguous int16 array of shape (N, H, W)")
            if Q is not None and (xyz is None or xyz.shape != (N, H, W, 3) or xyz.dtype != np.float32 or not xyz.flags.c_contiguous):
                raise error("compute_batch_host: out[1] must be a C-contiguous float32 array of shape (N, H, W, 3)")
        if disps is None:
            disps = np.empty((N, H, W), np.int16)
        qp = None
        if Q is not None:
            Q = np.ascontiguousarray(Q, np.float64)
            if xyz is None:
                xyz = np.empty((N, H, W, 3), np.float32)
            qp = Q.ctypes.data
        self._channels(cn)
        _check(self._L.sgm_compute_batch(self._h, N, lefts.ctypes.data, rights.ctypes.data, H, W, disps.ctypes.data,
                                         xyz.ctypes.data if Q is not None else None, qp))
        return (disps, xyz) if Q is not None else disps

    def disp_to_float_host(self, disp: np.ndarray) -> np.ndarray:
        disp = np.ascontiguousarray(disp, np.int16)
        out = np.empty(disp.shape, np.float32)
        _check(self._L.sgm_disp_to_float(self._h, disp.ctypes.data, disp.size, out.ctypes.data))
        return out

    def reproject_host(self, disp: np.ndarray, Q: np.ndarray, handle_missing: bool) -> np.ndarray:
        H, W = disp.shape
        out = np.empty((H, W, 3), np.float32)
        _check(self._L.sgm_reproject(self._h, disp.ctypes.data, H, W, Q.ctypes.data, int(handle_missing),
                                     out.ctypes.data))
        return out

    def compact_points_host(self, xyz: np.ndarray, disp: np.ndarray, colors: np.ndarray | None = None):
        """(points_3D[mask], colors[mask]) with the mask of main.ipynb:726-730, row-major order kept."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        disp = np.ascontiguousarray(disp, np.float32).reshape(-1)
        n = disp.size
        pts = np.empty((n, 3), np.float32)
        rgb = None
        cp = None
        if colors is not None:
            colors = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
            rgb = np.empty((n, 3), np.uint8)
            cp = colors.ctypes.data
        nv = C.c_int64(0)
        _check(self._L.sgm_compact_points(self._h, xyz.ctypes.data, disp.ctypes.data, cp, n, pts.ctypes.data,
                                          rgb.ctypes.data if rgb is not None else None, C.byref(nv)))
        return (pts[:nv.value].copy(), rgb[:nv.value].copy() if rgb is not None else None)

    def compact_points_device(self, d_xyz: int, d_dispf: int, d_colors: int | None, n: int, d_points: int,
                              d_out_colors: int | None) -> int:
        """Device-resident form (sgm_compact_points_device): valid points of one frame packed to the front of
        d_points, in row-major order; returns their number (synchronises the engine's stream)."""
        nv = C.c_int64(0)
        _check(self._L.sgm_compact_points_device(self._h, d_xyz, d_dispf, d_colors, n, d_points, d_out_colors, C.byref(nv)))
        return int(nv.value)

    def compact_points_device_async(self, d_xyz: int, d_dispf: int, d_colors: int | None, n: int, d_points: int,
                                    d_out_colors: int | None, d_count_i64: int) -> None:
        """The same in stream order (sgm_compact_points_device_async): the count goes to an int64 in DEVICE memory,
        nothing is synchronised."""
        _check(self._L.sgm_compact_points_device_async(self._h, d_xyz, d_dispf, d_colors, n, d_points, d_out_colors, d_count_i64))

    # -- voxel-grid downsampling (include/sgm_hip_voxel.h) --
    def voxel_downsample_host(self, xyz: np.ndarray, disp: np.ndarray | None, colors: np.ndarray | None, voxel_size: float,
                              origin=(0.0, 0.0, 0.0), min_points: int = 1, return_counts: bool = False):
        """sgm_voxel_downsample: float32 points (n, 3) or (H, W, 3), float32 disparities (n) or (H, W) or None, uint8 colours of
        the points' shape or None.  Returns (points float32 (M, 3), colors uint8 (M, 3) or None, counts uint32 (M) or None,
        n_out_of_range), the voxels in the order of their first points."""
        xyz, n, disp, colors = _cloud_in(xyz, disp, colors)
        org = _vec3(origin)
        pts = np.empty((n, 3), np.float32)
        rgb = None if colors is None else np.empty((n, 3), np.uint8)
        cnt = np.empty(n, np.uint32) if return_counts else None
        nv, noor = C.c_int64(0), C.c_int64(0)
        _check(self._L.sgm_voxel_downsample(self._h, xyz.ctypes.data, _at(disp), _at(colors), n, float(voxel_size), org.ctypes.data,
                                            int(min_points), pts.ctypes.data, _at(rgb), _at(cnt), C.byref(nv), C.byref(noor)))
        m = nv.value
        return (pts[:m].copy(), None if rgb is None else rgb[:m].copy(), None if cnt is None else cnt[:m].copy(), int(noor.value))

    def voxel_downsample_device(self, d_xyz: int, d_dispf: int | None, d_colors: int | None, n: int, voxel_size: float, origin,
                                min_points: int, d_points: int, d_out_colors: int | None = None, d_out_counts: int | None = None):
        """sgm_voxel_downsample_device: device addresses, outputs with room for n rows; the rows go to the front of the outputs in
        the order of the voxels' first points.  Returns (n_voxels, n_out_of_range); synchronises the engine's stream."""
        org = _vec3(origin)
        nv, noor = C.c_int64(0), C.c_int64(0)
        _check(self._L.sgm_voxel_downsample_device(self._h, d_xyz, d_dispf, d_colors, int(n), float(voxel_size), org.ctypes.data,
                                                   int(min_points), d_points, d_out_colors, d_out_counts, C.byref(nv), C.byref(noor)))
        return int(nv.value), int(noor.value)

    # -- radius outlier removal (include/sgm_hip_radius.h) --
    def radius_outlier_host(self, xyz: np.ndarray, disp: np.ndarray | None, colors: np.ndarray | None, radius: float, nb_points: int,
                            max_count: int | None = None, origin=(0.0, 0.0, 0.0), return_counts: bool = False,
                            return_index: bool = False):
        """sgm_radius_outlier: float32 points (n, 3) or (H, W, 3), float32 disparities (n) or (H, W) or None, uint8 colours of the
        points' shape or None; max_count None means nb_points.  Returns (points float32 (M, 3), colors uint8 (M, 3) or None,
        keep uint8 (n), counts uint32 (n) or None, index uint32 (M) or None, n_out_of_range): the kept points in source order."""
        xyz, n, disp, colors = _cloud_in(xyz, disp, colors)
        org = _vec3(origin)
        keep = np.zeros(n, np.uint8)
        cnt = np.zeros(n, np.uint32) if return_counts else None
        pts = np.empty((n, 3), np.float32)
        rgb = None if colors is None else np.empty((n, 3), np.uint8)
        idx = np.empty(n, np.uint32) if return_index else None
        nk, noor = C.c_int64(0), C.c_int64(0)
        _check(self._L.sgm_radius_outlier(self._h, xyz.ctypes.data, _at(disp), _at(colors), n, float(radius), org.ctypes.data,
                                          int(nb_points), int(nb_points if max_count is None else max_count), keep.ctypes.data,
                                          _at(cnt), pts.ctypes.data, _at(rgb), _at(idx), C.byref(nk), C.byref(noor)))
        m = nk.value
        return (pts[:m].copy(), None if rgb is None else rgb[:m].copy(), keep, cnt, None if idx is None else idx[:m].copy(),
                int(noor.value))

    def radius_outlier_device(self, d_xyz: int, d_dispf: int | None, d_colors: int | None, n: int, radius: float, nb_points: int,
                              max_count: int | None = None, origin=(0.0, 0.0, 0.0), d_keep: int | None = None,
                              d_counts: int | None = None, d_points: int | None = None, d_out_colors: int | None = None,
                              d_index: int | None = None):
        """sgm_radius_outlier_device: device addresses; d_keep (uint8) and d_counts (uint32) have n entries, d_points, d_out_colors
        and d_index (uint32) room for n rows, and the kept points go to their front in source order.  Returns (n_kept,
        n_out_of_range); synchronises the engine's stream."""
        org = _vec3(origin)
        nk, noor = C.c_int64(0), C.c_int64(0)
        _check(self._L.sgm_radius_outlier_device(self._h, d_xyz, d_dispf, d_colors, int(n), float(radius), org.ctypes.data,
                                                 int(nb_points), int(nb_points if max_count is None else max_count), d_keep, d_counts,
                                                 d_points, d_out_colors, d_index, C.byref(nk), C.byref(noor)))
        return int(nk.value), int(noor.value)

    # -- statistical outlier removal (include/sgm_hip_statistical.h) --
    def statistical_outlier_host(self, xyz: np.ndarray, disp: np.ndarray | None, colors: np.ndarray | None, nb_neighbors: int,
                                 std_ratio: float, max_radius: float, origin=(0.0, 0.0, 0.0), return_distances: bool = False,
                                 return_index: bool = False):
        """sgm_statistical_outlier: float32 points (n, 3) or (H, W, 3), float32 disparities (n) or (H, W) or None, uint8 colours of
        the points' shape or None.  Returns (points float32 (M, 3), colors uint8 (M, 3) or None, keep uint8 (n), mean float32 (n)
        or None, index uint32 (M) or None, stats uint64 (8)): the kept points in source order; stats is points in range, valid
        points out of range, dense, sparse, A, B, T, 0."""
        xyz, n, disp, colors = _cloud_in(xyz, disp, colors)
        org = _vec3(origin)
        keep = np.zeros(n, np.uint8)
        mean = np.full(n, -1, np.float32) if return_distances else None
        pts = np.empty((n, 3), np.float32)
        rgb = None if colors is None else np.empty((n, 3), np.uint8)
        idx = np.empty(n, np.uint32) if return_index else None
        nk, stats = C.c_int64(0), np.zeros(8, np.uint64)
        _check(self._L.sgm_statistical_outlier(self._h, xyz.ctypes.data, _at(disp), _at(colors), n, int(nb_neighbors), float(std_ratio),
                                               float(max_radius), org.ctypes.data, keep.ctypes.data, _at(mean), pts.ctypes.data, _at(rgb),
                                               _at(idx), C.byref(nk), stats.ctypes.data))
        m = nk.value
        return (pts[:m].copy(), None if rgb is None else rgb[:m].copy(), keep, mean, None if idx is None else idx[:m].copy(), stats)

    def statistical_outlier_device(self, d_xyz: int, d_dispf: int | None, d_colors: int | None, n: int, nb_neighbors: int,
                                   std_ratio: float, max_radius: float, origin=(0.0, 0.0, 0.0), d_keep: int | None = None,
                                   d_mean: int | None = None, d_points: int | None = None, d_out_colors: int | None = None,
                                   d_index: int | None = None):
        """sgm_statistical_outlier_device: device addresses; d_keep (uint8) and d_mean (float32) have n entries, d_points,
        d_out_colors and d_index (uint32) room for n rows, and the kept points go to their front in source order.  Returns
        (n_kept, stats uint64 (8)); synchronises the engine's stream."""
        org = _vec3(origin)
        nk, stats = C.c_int64(0), np.zeros(8, np.uint64)
        _check(self._L.sgm_statistical_outlier_device(self._h, d_xyz, d_dispf, d_colors, int(n), int(nb_neighbors), float(std_ratio),
                                                      float(max_radius), org.ctypes.data, d_keep, d_mean, d_points, d_out_colors, d_index,
                                                      C.byref(nk), stats.ctypes.data))
        return int(nk.value), stats

    # -- covariance normals of a point list (include/sgm_hip_covariance.h) --
    def covariance_normals_host(self, xyz: np.ndarray, disp: np.ndarray | None, radius: float, min_neighbors: int = 3,
                                origin=(0.0, 0.0, 0.0), viewpoint=(0.0, 0.0, 0.0), orient: bool = True,
                                return_curvature: bool = False, return_counts: bool = False):
        """sgm_covariance_normals: float32 points (n, 3) or (H, W, 3), float32 disparities (n) or (H, W) or None.  Returns (normals
        float32 (n, 3), curvature float32 (n) or None, counts uint32 (n) or None, stats uint64 (4)), all at the source index: a
        point without a normal has (0, 0, 0) and -1; stats is points in range, valid points out of range, points with a normal,
        degenerate points."""
        xyz, n, disp, _ = _cloud_in(xyz, disp, None)
        org = _vec3(origin)
        view = _vec3(viewpoint)
        nrm = np.zeros((n, 3), np.float32)
        curv = np.full(n, -1, np.float32) if return_curvature else None
        cnt = np.zeros(n, np.uint32) if return_counts else None
        stats = np.zeros(4, np.uint64)
        _check(self._L.sgm_covariance_normals(self._h, xyz.ctypes.data, _at(disp), n, float(radius), int(min_neighbors), org.ctypes.data,
                                              view.ctypes.data, int(bool(orient)), nrm.ctypes.data, _at(curv), _at(cnt), stats.ctypes.data))
        return nrm, curv, cnt, stats

    def covariance_normals_device(self, d_xyz: int, d_dispf: int | None, n: int, radius: float, min_neighbors: int = 3,
                                  origin=(0.0, 0.0, 0.0), viewpoint=(0.0, 0.0, 0.0), orient: bool = True, d_normals: int | None = None,
                                  d_curvature: int | None = None, d_counts: int | None = None, return_stats: bool = True):
        """sgm_covariance_normals_device: device addresses; d_normals (float32) has n rows of 3, d_curvature (float32) and d_counts
        (uint32) n entries.  Returns stats uint64 (4) after synchronising the engine's stream, or with return_stats=False None
        with the outputs complete once the stream has run (synchronize())."""
        org = _vec3(origin)
        view = _vec3(viewpoint)
        stats = np.zeros(4, np.uint64) if return_stats else None
        _check(self._L.sgm_covariance_normals_device(self._h, d_xyz, d_dispf, int(n), float(radius), int(min_neighbors), org.ctypes.data,
                                                     view.ctypes.data, int(bool(orient)), d_normals, d_curvature, d_counts,
                                                     None if stats is None else stats.ctypes.data))
        return stats

    # -- density clustering of the point cloud (include/sgm_hip_dbscan.h) --
    def cluster_dbscan_host(self, xyz: np.ndarray, disp: np.ndarray | None, eps: float, min_points: int, origin=(0.0, 0.0, 0.0),
                            return_core: bool = False, return_sizes: bool = False):
        """sgm_cluster_dbscan: float32 points (n, 3) or (H, W, 3), float32 disparities (n) or (H, W) or None.  Returns (labels int32
        (n): the cluster's number or -1, core uint8 (n) or None, sizes uint32 (clusters) or None, stats uint64 (6)), the first two at
        the source index; stats is points in range, valid points out of range, core, border, in-range noise, clusters."""
        xyz, n, disp, _ = _cloud_in(xyz, disp, None)
        org = _vec3(origin)
        labels = np.full(n, -1, np.int32)
        core = np.zeros(n, np.uint8) if return_core else None
        sizes = np.zeros(n, np.uint32) if return_sizes else None
        stats = np.zeros(6, np.uint64)
        nc = C.c_int64(0)
        _check(self._L.sgm_cluster_dbscan(self._h, xyz.ctypes.data, _at(disp), n, float(eps), int(min_points), org.ctypes.data,
                                          labels.ctypes.data, _at(core), _at(sizes), stats.ctypes.data, C.byref(nc)))
        return labels, core, None if sizes is None else sizes[:int(nc.value)].copy(), stats

    def cluster_dbscan_device(self, d_xyz: int, d_dispf: int | None, n: int, eps: float, min_points: int, origin=(0.0, 0.0, 0.0),
                              d_labels: int | None = None, d_core: int | None = None, d_sizes: int | None = None):
        """sgm_cluster_dbscan_device: device addresses; d_labels (int32) and d_core (uint8) have n entries, d_sizes (uint32) room for
        n of which the first `clusters` are written.  Returns (clusters, stats uint64 (6)) after synchronising the engine's stream."""
        org = _vec3(origin)
        stats = np.zeros(6, np.uint64)
        nc = C.c_int64(0)
        _check(self._L.sgm_cluster_dbscan_device(self._h, d_xyz, d_dispf, int(n), float(eps), int(min_points), org.ctypes.data,
                                                 d_labels, d_core, d_sizes, stats.ctypes.data, C.byref(nc)))
        return int(nc.value), stats

    # -- plane segmentation of the point cloud (include/sgm_hip_plane.h) --
    @staticmethod
    def _plane_host_args(xyz, disp, colors, return_distances, return_points, return_index):
        xyz, n, disp, colors = _cloud_in(xyz, disp, colors)
        inl = np.zeros(n, np.uint8)
        dist = np.full(n, np.nan, np.float32) if return_distances else None
        pts = np.empty((n, 3), np.float32) if return_points else None
        rgb = np.empty((n, 3), np.uint8) if return_points and colors is not None else None
        idx = np.empty(n, np.uint32) if return_index else None
        return xyz, n, disp, colors, inl, dist, pts, rgb, idx

    def segment_plane_host(self, xyz: np.ndarray, disp: np.ndarray | None, colors: np.ndarray | None, distance_threshold: float,
                           num_iterations: int = 1000, seed: int = 0, refine: bool = True, select: int = 0,
                           return_distances: bool = False, return_points: bool = True, return_index: bool = False):
        """sgm_segment_plane: float32 points (n, 3) or (H, W, 3), float32 disparities (n) or (H, W) or None, uint8 colours of the
        points' shape or None.  Returns (model float32 (4), inlier uint8 (n), distances float32 (n) or None, points float32 (M, 3)
        or None, colors uint8 (M, 3) or None, index uint32 (M) or None, stats uint64 (8), n_inliers): the M selected points --
        the inliers (select 0) or the valid points off the plane (select 1) -- in source order; stats is valid points, degenerate
        hypotheses, k*, its count, inliers in refit range, inliers out of it, refined, found."""
        xyz, n, disp, colors, inl, dist, pts, rgb, idx = self._plane_host_args(xyz, disp, colors, return_distances, return_points,
                                                                               return_index)
        model, stats = np.zeros(4, np.float32), np.zeros(8, np.uint64)
        ni, ns = C.c_int64(0), C.c_int64(0)
        _check(self._L.sgm_segment_plane(self._h, xyz.ctypes.data, _at(disp), _at(colors), n, float(distance_threshold), int(num_iterations),
                                         int(seed), int(bool(refine)), int(select), inl.ctypes.data, _at(dist), _at(pts), _at(rgb), _at(idx),
                                         model.ctypes.data, stats.ctypes.data, C.byref(ni), C.byref(ns)))
        cut = lambda a: None if a is None else a[:ns.value].copy()
        return model, inl, dist, cut(pts), cut(rgb), cut(idx), stats, int(ni.value)

    def segment_plane_device(self, d_xyz: int, d_dispf: int | None, d_colors: int | None, n: int, distance_threshold: float,
                             num_iterations: int = 1000, seed: int = 0, refine: bool = True, select: int = 0,
                             d_inlier: int | None = None, d_distance: int | None = None, d_points: int | None = None,
                             d_out_colors: int | None = None, d_index: int | None = None):
        """sgm_segment_plane_device: device addresses; d_inlier (uint8) and d_distance (float32) have n entries, d_points,
        d_out_colors and d_index (uint32) room for n rows, and the selected points go to their front in source order.  Returns
        (model float32 (4), stats uint64 (8), n_inliers, n_selected) after synchronising the engine's stream, once."""
        model, stats = np.zeros(4, np.float32), np.zeros(8, np.uint64)
        ni, ns = C.c_int64(0), C.c_int64(0)
        _check(self._L.sgm_segment_plane_device(self._h, d_xyz, d_dispf, d_colors, int(n), float(distance_threshold), int(num_iterations),
                                                int(seed), int(bool(refine)), int(select), d_inlier, d_distance, d_points, d_out_colors,
                                                d_index, model.ctypes.data, stats.ctypes.data, C.byref(ni), C.byref(ns)))
        return model, stats, int(ni.value), int(ns.value)

    def plane_inliers_host(self, xyz: np.ndarray, disp: np.ndarray | None, colors: np.ndarray | None, plane_model,
                           distance_threshold: float, select: int = 0, return_distances: bool = False, return_points: bool = True,
                           return_index: bool = False):
        """sgm_plane_inliers: step 8 of sgm_segment_plane on the caller's model (a, b, c, d).  Returns (inlier uint8 (n), distances
        float32 (n) or None, points float32 (M, 3) or None, colors uint8 (M, 3) or None, index uint32 (M) or None, n_inliers)."""
        xyz, n, disp, colors, inl, dist, pts, rgb, idx = self._plane_host_args(xyz, disp, colors, return_distances, return_points,
                                                                               return_index)
        model = np.ascontiguousarray(plane_model, np.float32).reshape(4)
        ni, ns = C.c_int64(0), C.c_int64(0)
        _check(self._L.sgm_plane_inliers(self._h, xyz.ctypes.data, _at(disp), _at(colors), n, model.ctypes.data, float(distance_threshold),
                                         int(select), inl.ctypes.data, _at(dist), _at(pts), _at(rgb), _at(idx), C.byref(ni), C.byref(ns)))
        cut = lambda a: None if a is None else a[:ns.value].copy()
        return inl, dist, cut(pts), cut(rgb), cut(idx), int(ni.value)

    def plane_inliers_device(self, d_xyz: int, d_dispf: int | None, d_colors: int | None, n: int, plane_model, distance_threshold: float,
                             select: int = 0, d_inlier: int | None = None, d_distance: int | None = None, d_points: int | None = None,
                             d_out_colors: int | None = None, d_index: int | None = None):
        """sgm_plane_inliers_device: device addresses as in segment_plane_device.  Returns (n_inliers, n_selected) after
        synchronising the engine's stream."""
        model = np.ascontiguousarray(plane_model, np.float32).reshape(4)
        ni, ns = C.c_int64(0), C.c_int64(0)
        _check(self._L.sgm_plane_inliers_device(self._h, d_xyz, d_dispf, d_colors, int(n), model.ctypes.data, float(distance_threshold),
                                                int(select), d_inlier, d_distance, d_points, d_out_colors, d_index, C.byref(ni),
                                                C.byref(ns)))
        return int(ni.value), int(ns.value)

    # -- rigid registration of two point clouds (include/sgm_hip_icp.h) --
    @staticmethod
    def _icp_small(max_iteration):
        """the small host results of a registration call: (T, fitness, rmse, history pre-filled with NaN, stats)"""
        return (np.zeros(16, np.float64), C.c_double(0.0), C.c_double(0.0), np.full((int(max_iteration) + 1, 2), np.nan, np.float64),
                np.zeros(8, np.uint64))

    def register_icp_host(self, source: np.ndarray, source_disp: np.ndarray | None, target: np.ndarray, target_disp: np.ndarray | None,
                          target_normals: np.ndarray | None, max_correspondence_distance: float, origin=(0.0, 0.0, 0.0), init=None,
                          estimation: int = 1, max_iteration: int = 30, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6):
        """sgm_register_icp: float32 points (n, 3) or (H, W, 3) and float32 disparities (n) or (H, W) or None for both clouds, float32
        normals of the target's shape or None.  Returns (T float64 (4, 4), fitness, rmse, corr int32 (ns), d2 float32 (ns), history
        float64 (evaluations, 2), stats uint64 (8)): stats is valid source points, target points in range, valid target points out
        of range, iterations, correspondences, unplaced, unusable normals, status."""
        src, ns, ds, _ = _cloud_in(source, source_disp, None)
        tgt, nt, dt, _ = _cloud_in(target, target_disp, None)
        nrm = None if target_normals is None else np.ascontiguousarray(target_normals, np.float32).reshape(-1, 3)
        org = _vec3(origin)
        T0 = np.ascontiguousarray(np.eye(4) if init is None else init, np.float64).reshape(16)
        T, fit, rmse, hist, stats = self._icp_small(max_iteration)
        corr, d2 = np.full(ns, -1, np.int32), np.full(ns, np.nan, np.float32)
        _check(self._L.sgm_register_icp(self._h, src.ctypes.data, _at(ds), ns, tgt.ctypes.data, _at(dt), _at(nrm), nt,
                                        float(max_correspondence_distance), org.ctypes.data, T0.ctypes.data, int(estimation),
                                        int(max_iteration), float(relative_fitness), float(relative_rmse), T.ctypes.data, C.byref(fit),
                                        C.byref(rmse), corr.ctypes.data, d2.ctypes.data, hist.ctypes.data, stats.ctypes.data))
        return T.reshape(4, 4), fit.value, rmse.value, corr, d2, hist[:int(stats[3]) + 1].copy(), stats

    def register_icp_device(self, d_source: int, d_source_disp: int | None, ns: int, d_target: int, d_target_disp: int | None,
                            d_target_normals: int | None, nt: int, max_correspondence_distance: float, origin=(0.0, 0.0, 0.0), init=None,
                            estimation: int = 1, max_iteration: int = 30, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6,
                            d_corr: int | None = None, d_d2: int | None = None):
        """sgm_register_icp_device: device addresses; d_corr (int32) and d_d2 (float32) have ns entries.  Returns (T float64 (4, 4),
        fitness, rmse, history float64 (evaluations, 2), stats uint64 (8)); synchronises the engine's stream once for the target's
        grid and once per evaluation."""
        org = _vec3(origin)
        T0 = np.ascontiguousarray(np.eye(4) if init is None else init, np.float64).reshape(16)
        T, fit, rmse, hist, stats = self._icp_small(max_iteration)
        _check(self._L.sgm_register_icp_device(self._h, d_source, d_source_disp, int(ns), d_target, d_target_disp, d_target_normals, int(nt),
                                               float(max_correspondence_distance), org.ctypes.data, T0.ctypes.data, int(estimation),
                                               int(max_iteration), float(relative_fitness), float(relative_rmse), T.ctypes.data,
                                               C.byref(fit), C.byref(rmse), d_corr, d_d2, hist.ctypes.data, stats.ctypes.data))
        return T.reshape(4, 4), fit.value, rmse.value, hist[:int(stats[3]) + 1].copy(), stats

    def evaluate_registration_host(self, source: np.ndarray, source_disp: np.ndarray | None, target: np.ndarray,
                                   target_disp: np.ndarray | None, max_correspondence_distance: float, origin=(0.0, 0.0, 0.0),
                                   transformation=None):
        """sgm_evaluate_registration: the correspondence pass alone under `transformation` (None: the identity).  Returns (fitness,
        rmse, corr int32 (ns), d2 float32 (ns), stats uint64 (8))."""
        src, ns, ds, _ = _cloud_in(source, source_disp, None)
        tgt, nt, dt, _ = _cloud_in(target, target_disp, None)
        org = _vec3(origin)
        T = np.ascontiguousarray(np.eye(4) if transformation is None else transformation, np.float64).reshape(16)
        fit, rmse, stats = C.c_double(0.0), C.c_double(0.0), np.zeros(8, np.uint64)
        corr, d2 = np.full(ns, -1, np.int32), np.full(ns, np.nan, np.float32)
        _check(self._L.sgm_evaluate_registration(self._h, src.ctypes.data, _at(ds), ns, tgt.ctypes.data, _at(dt), nt,
                                                 float(max_correspondence_distance), org.ctypes.data, T.ctypes.data, C.byref(fit),
                                                 C.byref(rmse), corr.ctypes.data, d2.ctypes.data, stats.ctypes.data))
        return fit.value, rmse.value, corr, d2, stats

    def evaluate_registration_device(self, d_source: int, d_source_disp: int | None, ns: int, d_target: int, d_target_disp: int | None,
                                     nt: int, max_correspondence_distance: float, origin=(0.0, 0.0, 0.0), transformation=None,
                                     d_corr: int | None = None, d_d2: int | None = None):
        """sgm_evaluate_registration_device: device addresses as in register_icp_device.  Returns (fitness, rmse, stats uint64 (8))."""
        org = _vec3(origin)
        T = np.ascontiguousarray(np.eye(4) if transformation is None else transformation, np.float64).reshape(16)
        fit, rmse, stats = C.c_double(0.0), C.c_double(0.0), np.zeros(8, np.uint64)
        _check(self._L.sgm_evaluate_registration_device(self._h, d_source, d_source_disp, int(ns), d_target, d_target_disp, int(nt),
                                                        float(max_correspondence_distance), org.ctypes.data, T.ctypes.data, C.byref(fit),
                                                        C.byref(rmse), d_corr, d_d2, stats.ctypes.data))
        return fit.value, rmse.value, stats

    def transform_points_host(self, xyz: np.ndarray, transformation, normals: np.ndarray | None = None):
        """sgm_transform_points: float32 points of any shape (..., 3) under the float64 4 x 4 transformation, the normals by its
        rotation part.  Returns (points, normals or None) of the inputs' shapes."""
        pts = np.ascontiguousarray(xyz, np.float32)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32)
        T = np.ascontiguousarray(transformation, np.float64).reshape(16)
        out, out_n = np.empty_like(pts), None if nrm is None else np.empty_like(nrm)
        _check(self._L.sgm_transform_points(self._h, pts.ctypes.data, _at(nrm), pts.size // 3, T.ctypes.data, out.ctypes.data, _at(out_n)))
        return out, out_n

    def transform_points_device(self, d_xyz: int, d_normals: int | None, n: int, transformation, d_out_xyz: int | None,
                                d_out_normals: int | None = None):
        """sgm_transform_points_device: device addresses (the outputs may be the inputs); enqueued on the engine's stream, which
        synchronize() waits for."""
        T = np.ascontiguousarray(transformation, np.float64).reshape(16)
        _check(self._L.sgm_transform_points_device(self._h, d_xyz, d_normals, int(n), T.ctypes.data, d_out_xyz, d_out_normals))

    # -- the truncated signed distance volume (include/sgm_hip_tsdf.h) --
    def tsdf_integrate_host(self, dims, voxel_size, sdf_trunc, origin, sum_, weight, rgb_sum, xyz, disp, colors, cam, front, extrinsic,
                            max_depth=float("inf"), stats=False):
        """sgm_tsdf_integrate: one frame into the planes, IN PLACE (int32 (V) sum and weight, uint32 (3, V) rgb_sum or None, all
        C-contiguous numpy arrays); xyz float32 (H, W, 3), disp float32 (H, W) or None, colors uint8 (H, W, 3) iff rgb_sum.
        Returns the eight counts (uint64) with stats, else None."""
        d = np.ascontiguousarray(dims, np.int32).reshape(3)
        org, cam4 = _vec3(origin), np.ascontiguousarray(cam, np.float32).reshape(4)
        T = np.ascontiguousarray(extrinsic, np.float64).reshape(16)
        xyz = np.ascontiguousarray(xyz, np.float32)
        H, W = xyz.shape[:2]
        disp = None if disp is None else np.ascontiguousarray(disp, np.float32)
        colors = None if colors is None else np.ascontiguousarray(colors, np.uint8)
        st = np.zeros(8, np.uint64) if stats else None
        _check(self._L.sgm_tsdf_integrate(self._h, d.ctypes.data, float(voxel_size), float(sdf_trunc), org.ctypes.data, _at(sum_), _at(weight),
                                          _at(rgb_sum), xyz.ctypes.data, _at(disp), _at(colors), H, W, cam4.ctypes.data, int(front),
                                          T.ctypes.data, float(max_depth), _at(st)))
        return st

    def tsdf_integrate_device(self, dims, voxel_size, sdf_trunc, origin, d_sum: int, d_weight: int, d_rgb_sum: int | None, d_xyz: int,
                              d_disp: int | None, d_colors: int | None, H: int, W: int, cam, front, extrinsic, max_depth=float("inf"),
                              stats=False):
        """sgm_tsdf_integrate_device: device addresses; enqueued on the engine's stream, which it waits for only with stats."""
        d = np.ascontiguousarray(dims, np.int32).reshape(3)
        org, cam4 = _vec3(origin), np.ascontiguousarray(cam, np.float32).reshape(4)
        T = np.ascontiguousarray(extrinsic, np.float64).reshape(16)
        st = np.zeros(8, np.uint64) if stats else None
        _check(self._L.sgm_tsdf_integrate_device(self._h, d.ctypes.data, float(voxel_size), float(sdf_trunc), org.ctypes.data, d_sum, d_weight,
                                                 d_rgb_sum, d_xyz, d_disp, d_colors, int(H), int(W), cam4.ctypes.data, int(front),
                                                 T.ctypes.data, float(max_depth), _at(st)))
        return st

    def tsdf_extract_host(self, dims, voxel_size, origin, sum_, weight, rgb_sum, min_weight=1, out_points=None, out_colors=None):
        """sgm_tsdf_extract_points: the number of crossings; rows go to out_points float32 (capacity, 3) and out_colors uint8
        (capacity, 3) if given (min(total, capacity) of them; the others stay as they are)."""
        d = np.ascontiguousarray(dims, np.int32).reshape(3)
        org = _vec3(origin)
        cap = 0 if out_points is None else out_points.shape[0]
        total = C.c_int64(-1)
        _check(self._L.sgm_tsdf_extract_points(self._h, d.ctypes.data, float(voxel_size), org.ctypes.data, _at(sum_), _at(weight), _at(rgb_sum),
                                               int(min_weight), cap, _at(out_points), _at(out_colors), C.byref(total)))
        return total.value

    def tsdf_extract_device(self, dims, voxel_size, origin, d_sum: int, d_weight: int, d_rgb_sum: int | None, min_weight=1, capacity=0,
                            d_out_points: int | None = None, d_out_colors: int | None = None):
        """sgm_tsdf_extract_points_device: device addresses; blocks once, returns the number of crossings."""
        d = np.ascontiguousarray(dims, np.int32).reshape(3)
        org = _vec3(origin)
        total = C.c_int64(-1)
        _check(self._L.sgm_tsdf_extract_points_device(self._h, d.ctypes.data, float(voxel_size), org.ctypes.data, d_sum, d_weight, d_rgb_sum,
                                                      int(min_weight), int(capacity), d_out_points, d_out_colors, C.byref(total)))
        return total.value

    # -- triangle mesh from the organised cloud (include/sgm_hip_mesh.h) --
    def mesh_grid_host(self, xyz: np.ndarray, disp: np.ndarray, colors: np.ndarray | None, max_diff: float = 1.0):
        """sgm_mesh_grid: float32 points (H, W, 3), float32 disparities (H, W), uint8 colours (H, W, 3) or None.  Returns
        (vertices float32 (V, 3), colors uint8 (V, 3) or None, faces int32 (F, 3)): the vertices in row-major order of their
        pixels, the faces in row-major order of their quads."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        H, W = xyz.shape[:2]
        disp = np.ascontiguousarray(disp, np.float32).reshape(H, W)
        colors = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(H, W, 3)
        vert = np.empty((H * W, 3), np.float32)
        rgb = None if colors is None else np.empty((H * W, 3), np.uint8)
        faces = np.empty((2 * max(H - 1, 0) * max(W - 1, 0), 3), np.int32)
        nv, nf = C.c_int64(0), C.c_int64(0)
        _check(self._L.sgm_mesh_grid(self._h, xyz.ctypes.data, disp.ctypes.data, _at(colors), H, W, float(max_diff), vert.ctypes.data,
                                     _at(rgb), faces.ctypes.data, C.byref(nv), C.byref(nf)))
        return vert[:nv.value].copy(), None if rgb is None else rgb[:nv.value].copy(), faces[:nf.value].copy()

    def mesh_grid_device(self, d_xyz: int, d_dispf: int, d_colors: int | None, H: int, W: int, max_diff: float, d_vertices: int,
                         d_out_colors: int | None, d_faces: int):
        """sgm_mesh_grid_device: device addresses, outputs with room for H * W vertex rows and 2 (H - 1)(W - 1) face rows; the rows
        go to the front of the outputs.  Returns (n_vertices, n_faces); synchronises the engine's stream."""
        nv, nf = C.c_int64(0), C.c_int64(0)
        _check(self._L.sgm_mesh_grid_device(self._h, d_xyz, d_dispf, d_colors, int(H), int(W), float(max_diff), d_vertices, d_out_colors,
                                            d_faces, C.byref(nv), C.byref(nf)))
        return int(nv.value), int(nf.value)

    # -- vertex normals of that mesh, and the normal image (include/sgm_hip_normals.h) --
    def normals_grid_host(self, xyz: np.ndarray, disp: np.ndarray, max_diff: float = 1.0, orient: bool = True) -> np.ndarray:
        """sgm_normals_grid: float32 points (H, W, 3) and disparities (H, W).  Returns the normal image float32 (H, W, 3): unit
        normals at the pixels that are vertices of the grid mesh, (0, 0, 0) elsewhere; with orient turned towards the camera."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        H, W = xyz.shape[:2]
        disp = np.ascontiguousarray(disp, np.float32).reshape(H, W)
        out = np.empty((H, W, 3), np.float32)
        _check(self._L.sgm_normals_grid(self._h, xyz.ctypes.data, disp.ctypes.data, H, W, float(max_diff), int(orient), out.ctypes.data))
        return out

    def normals_grid_device(self, d_xyz: int, d_dispf: int, H: int, W: int, max_diff: float, orient: bool, d_normals: int) -> None:
        """sgm_normals_grid_device: device addresses, d_normals with room for H * W rows; in stream order, nothing is
        synchronised."""
        _check(self._L.sgm_normals_grid_device(self._h, d_xyz, d_dispf, int(H), int(W), float(max_diff), int(orient), d_normals))

    def mesh_grid_normals_host(self, xyz: np.ndarray, disp: np.ndarray, colors: np.ndarray | None, max_diff: float = 1.0,
                               orient: bool = True):
        """sgm_mesh_grid_normals: mesh_grid_host and one normal per vertex.  Returns (vertices float32 (V, 3), colors uint8 (V, 3)
        or None, faces int32 (F, 3), normals float32 (V, 3))."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        H, W = xyz.shape[:2]
        disp = np.ascontiguousarray(disp, np.float32).reshape(H, W)
        colors = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(H, W, 3)
        vert, nrm = np.empty((H * W, 3), np.float32), np.empty((H * W, 3), np.float32)
        rgb = None if colors is None else np.empty((H * W, 3), np.uint8)
        faces = np.empty((2 * max(H - 1, 0) * max(W - 1, 0), 3), np.int32)
        nv, nf = C.c_int64(0), C.c_int64(0)
        _check(self._L.sgm_mesh_grid_normals(self._h, xyz.ctypes.data, disp.ctypes.data, _at(colors), H, W, float(max_diff), int(orient),
                                             vert.ctypes.data, _at(rgb), faces.ctypes.data, nrm.ctypes.data, C.byref(nv), C.byref(nf)))
        return vert[:nv.value].copy(), None if rgb is None else rgb[:nv.value].copy(), faces[:nf.value].copy(), nrm[:nv.value].copy()

    def mesh_grid_normals_device(self, d_xyz: int, d_dispf: int, d_colors: int | None, H: int, W: int, max_diff: float, orient: bool,
                                 d_vertices: int, d_out_colors: int | None, d_faces: int, d_normals: int):
        """sgm_mesh_grid_normals_device: mesh_grid_device with d_normals, room for H * W rows like d_vertices.  Returns
        (n_vertices, n_faces); synchronises the engine's stream."""
        nv, nf = C.c_int64(0), C.c_int64(0)
        _check(self._L.sgm_mesh_grid_normals_device(self._h, d_xyz, d_dispf, d_colors, int(H), int(W), float(max_diff), int(orient),
                                                    d_vertices, d_out_colors, d_faces, d_normals, C.byref(nv), C.byref(nf)))
        return int(nv.value), int(nf.value)

    def median3x3_host(self, img: np.ndarray) -> np.ndarray:
        img = np.ascontiguousarray(img, np.int16)
        out = np.empty_like(img)
        _check(self._L.sgm_median3x3(self._h, img.ctypes.data, img.shape[0], img.shape[1], out.ctypes.data))
        return out

    def filter_speckles_host(self, img: np.ndarray, newVal: int, maxSpeckleSize: int, maxDiff: int) -> np.ndarray:
        out = np.array(img, dtype=np.int16, order="C", copy=True)
        _check(self._L.sgm_filter_speckles(self._h, out.ctypes.data, out.shape[0], out.shape[1], int(newVal),
                                           int(maxSpeckleSize), int(maxDiff)))
        return out

    def valid_mask_host(self, xyz: np.ndarray, disp: np.ndarray) -> np.ndarray:
        xyz = np.ascontiguousarray(xyz, np.float32)
        disp = np.ascontiguousarray(disp, np.float32)
        out = np.empty(disp.shape, np.uint8)
        _check(self._L.sgm_valid_mask(self._h, xyz.ctypes.data, disp.ctypes.data, disp.size, out.ctypes.data))
        return out.astype(bool)

    # -- device-pointer path (raw addresses; torch only supplies the memory)
    def _bind(self, fn, ptrs) -> None:
        n = len(ptrs)
        arr = (C.c_void_p * n)(*[int(x) if x else None for x in ptrs]) if n else None
        _check(fn(self._h, n, arr))

    def bind_confidence_device(self, ptrs) -> None:
        """Device addresses of tight uint8 (H, W) maps for the NEXT image call on this engine (sgm_bind_confidence_device;
        needs SGM_OPT_CONFIDENCE = 1): pair i's final confidence goes to ptrs[i].  An empty sequence clears the binding."""
        self._bind(self._L.sgm_bind_confidence_device, ptrs)

    def bind_right_device(self, ptrs) -> None:
        """Device addresses of tight int16 (H, W) maps for the NEXT image call on this engine (sgm_bind_right_device; needs
        SGM_OPT_RIGHT_VIEW = 1): pair i's final right-view map goes to ptrs[i].  An empty sequence clears the binding."""
        self._bind(self._L.sgm_bind_right_device, ptrs)

    # (cn: interleaved channels of the images, 1 or 3; stride is the row pitch in bytes; d_conf / d_confs: where the
    #  confidence maps of the call go, bind_confidence_device; d_rmap / d_rmaps: the right-view maps, bind_right_device)
    def compute_device(self, d_left: int, d_right: int, H: int, W: int, stride: int, d_disp: int, cn: int = 1,
                       d_conf: int | None = None, d_rmap: int | None = None) -> None:
        self._channels(cn)
        if d_conf is not None:
            self.bind_confidence_device([d_conf])
        if d_rmap is not None:
            self.bind_right_device([d_rmap])
        _check(self._L.sgm_compute_device(self._h, d_left, d_right, H, W, stride, d_disp))

    def pipeline_device(self, d_left: int, d_right: int, H: int, W: int, stride: int, Q: np.ndarray | None,
                        d_disp: int | None, d_dispf: int | None, d_xyz: int | None, cn: int = 1,
                        d_conf: int | None = None, d_rmap: int | None = None) -> None:
        qp = None
        if Q is not None:
            Q = np.ascontiguousarray(Q, np.float64)
            qp = Q.ctypes.data
        self._channels(cn)
        if d_conf is not None:
            self.bind_confidence_device([d_conf])
        if d_rmap is not None:
            self.bind_right_device([d_rmap])
        _check(self._L.sgm_pipeline_device(self._h, d_left, d_right, H, W, stride, qp, d_disp, d_dispf, d_xyz))

    def pipeline_batch_device(self, d_lefts, d_rights, H: int, W: int, stride: int, Q: np.ndarray | None,
                              d_disps, d_dispfs=None, d_xyzs=None, cn: int = 1, d_confs=None, d_rmaps=None) -> None:
        """N resident pairs in throughput mode (sgm_pipeline_batch_device): sequences of N device addresses.
        With SGM_OPT_SCHEDULE = 2 the pairs share one chained sweep launch per pass.  Asynchronous."""
        n = len(d_lefts)
        arr = lambda xs: (C.c_void_p * n)(*[int(x) for x in xs]) if xs is not None else None
        qp = None
        if Q is not None:
            Q = np.ascontiguousarray(Q, np.float64)
            qp = Q.ctypes.data
        a, b, c, d, f = arr(d_lefts), arr(d_rights), arr(d_disps), arr(d_dispfs), arr(d_xyzs)
        self._channels(cn)
        if d_confs is not None:
            self.bind_confidence_device(list(d_confs))
        if d_rmaps is not None:
            self.bind_right_device(list(d_rmaps))
        _check(self._L.sgm_pipeline_batch_device(self._h, n, a, b, H, W, stride, qp, c, d, f))

    def disp_to_float_device(self, d_disp: int, n: int, d_out: int) -> None:
        _check(self._L.sgm_disp_to_float_device(self._h, d_disp, n, d_out))

    def reproject_device(self, d_disp: int, H: int, W: int, Q: np.ndarray, handle_missing: bool, d_xyz: int) -> None:
        Q = np.ascontiguousarray(Q, np.float64)
        _check(self._L.sgm_reproject_device(self._h, d_disp, H, W, Q.ctypes.data, int(handle_missing), d_xyz))

    # -- rectification in front of the path (gui.py:160-164) --
    @staticmethod
    def _rectify_args(K, dist, R, P):
        K = np.ascontiguousarray(K, np.float64).reshape(3, 3)
        d = None if dist is None else np.ascontiguousarray(dist, np.float64).ravel()
        Rm = None if R is None else np.ascontiguousarray(R, np.float64).reshape(3, 3)
        Pm = None if P is None else np.ascontiguousarray(P, np.float64)
        if Pm is not None and Pm.shape not in ((3, 3), (3, 4)):
            raise error("initUndistortRectifyMap: newCameraMatrix must be 3x3 or 3x4")
        return K, d, Rm, Pm

    def init_undistort_rectify_map_host(self, K, dist, R, P, W: int, H: int):
        K, d, Rm, Pm = self._rectify_args(K, dist, R, P)
        m1 = np.empty((H, W), np.float32)
        m2 = np.empty((H, W), np.float32)
        _check(self._L.sgm_init_undistort_rectify_map(
            self._h, K.ctypes.data, None if d is None else d.ctypes.data, 0 if d is None else d.size,
            None if Rm is None else Rm.ctypes.data, None if Pm is None else Pm.ctypes.data,
            0 if Pm is None else Pm.shape[1], W, H, m1.ctypes.data, m2.ctypes.data))
        return m1, m2

    def init_undistort_rectify_map_device(self, K, dist, R, P, W: int, H: int, d_map1: int, d_map2: int) -> None:
        K, d, Rm, Pm = self._rectify_args(K, dist, R, P)
        _check(self._L.sgm_init_undistort_rectify_map_device(
            self._h, K.ctypes.data, None if d is None else d.ctypes.data, 0 if d is None else d.size,
            None if Rm is None else Rm.ctypes.data, None if Pm is None else Pm.ctypes.data,
            0 if Pm is None else Pm.shape[1], W, H, d_map1, d_map2))

    def remap_linear_host(self, src: np.ndarray, map1: np.ndarray, map2: np.ndarray) -> np.ndarray:
        cn = 1 if src.ndim == 2 else src.shape[2]
        dH, dW = map1.shape
        out = np.empty((dH, dW) if src.ndim == 2 else (dH, dW, cn), np.uint8)
        _check(self._L.sgm_remap_linear_u8(self._h, src.ctypes.data, src.shape[0], src.shape[1], src.strides[0], cn,
                                           map1.ctypes.data, map2.ctypes.data, dH, dW, out.ctypes.data))
        return out

    def remap_linear_device(self, d_src: int, sH: int, sW: int, sstride: int, cn: int, d_map1: int, d_map2: int,
                            dH: int, dW: int, d_dst: int, dstride: int) -> None:
        _check(self._L.sgm_remap_linear_u8_device(self._h, d_src, sH, sW, sstride, cn, d_map1, d_map2, dH, dW, d_dst, dstride))

    def valid_mask_device(self, d_xyz: int, d_disp: int, n: int, d_mask: int) -> None:
        _check(self._L.sgm_valid_mask_device(self._h, d_xyz, d_disp, n, d_mask))

    # -- the edge-aware disparity filter (include/sgm_hip_wls.h) --
    def wls_filter_host(self, disp: np.ndarray, guide: np.ndarray, conf: np.ndarray | None, invalid: int, lambda_: float,
                        lut: np.ndarray, return_float: bool = False):
        """sgm_wls_filter: int16 (H, W) map, uint8 (H, W) or (H, W, 3) guide, uint8 (H, W) confidence or None, the 256 float32
        edge weights; returns the filtered int16 map, or (map, float32 map in pixels) with return_float."""
        disp = np.ascontiguousarray(disp, np.int16)
        guide = np.ascontiguousarray(guide, np.uint8)
        conf = None if conf is None else np.ascontiguousarray(conf, np.uint8)
        lut = np.ascontiguousarray(lut, np.float32)
        H, W = disp.shape
        out = np.empty((H, W), np.int16)
        outf = np.empty((H, W), np.float32) if return_float else None
        _check(self._L.sgm_wls_filter(self._h, disp.ctypes.data, guide.ctypes.data, 1 if guide.ndim == 2 else guide.shape[2],
                                      None if conf is None else conf.ctypes.data, H, W, int(invalid), float(lambda_),
                                      lut.ctypes.data, out.ctypes.data, None if outf is None else outf.ctypes.data))
        return (out, outf) if return_float else out

    def wls_filter_device(self, d_disp: int, d_guide: int, cn: int, d_conf: int | None, H: int, W: int, invalid: int,
                          lambda_: float, lut: np.ndarray, d_out: int, d_out_f32: int | None = None) -> None:
        """sgm_wls_filter_device: device addresses (lut stays a host array), in the order of the engine's stream."""
        lut = np.ascontiguousarray(lut, np.float32)
        _check(self._L.sgm_wls_filter_device(self._h, d_disp, d_guide, int(cn), d_conf, H, W, int(invalid), float(lambda_),
                                             lut.ctypes.data, d_out, d_out_f32))

    # -- ... and its batch form (include/sgm_hip_wls_batch.h): N maps of one shape per call --
    def wls_filter_batch_host(self, disps: np.ndarray, guides: np.ndarray, confs: np.ndarray | None, invalid: int, lambda_: float,
                              lut: np.ndarray, return_float: bool = False):
        """sgm_wls_filter_batch: int16 (N, H, W) maps, uint8 (N, H, W) or (N, H, W, 3) guides, uint8 (N, H, W) confidence maps or
        None, the 256 float32 edge weights; returns the filtered int16 stack, or (stack, float32 stack in pixels) with
        return_float."""
        disps = np.ascontiguousarray(disps, np.int16)
        guides = np.ascontiguousarray(guides, np.uint8)
        confs = None if confs is None else np.ascontiguousarray(confs, np.uint8)
        lut = np.ascontiguousarray(lut, np.float32)
        N, H, W = disps.shape
        out = np.empty((N, H, W), np.int16)
        outf = np.empty((N, H, W), np.float32) if return_float else None
        _check(self._L.sgm_wls_filter_batch(self._h, N, disps.ctypes.data, guides.ctypes.data, 1 if guides.ndim == 3 else guides.shape[3],
                                            None if confs is None else confs.ctypes.data, H, W, int(invalid), float(lambda_),
                                            lut.ctypes.data, out.ctypes.data, None if outf is None else outf.ctypes.data))
        return (out, outf) if return_float else out

    def wls_filter_batch_device(self, d_disps, d_guides, cn: int, d_confs, H: int, W: int, invalid: int, lambda_: float,
                                lut: np.ndarray, d_outs, d_out_f32s=None) -> None:
        """sgm_wls_filter_batch_device: sequences of N device addresses (d_confs / d_out_f32s: such a sequence, or None for none;
        lut stays a host array), in the order of the engine's stream."""
        n = len(d_disps)
        arr = lambda xs: (C.c_void_p * len(xs))(*[int(x) if x else None for x in xs]) if xs is not None and len(xs) else None
        for xs in (d_guides, d_confs, d_outs, d_out_f32s):
            if xs is not None and len(xs) != n:
                raise error(f"wls_filter_batch_device: {n} maps, but a sequence of {len(xs)} addresses")
        lut = np.ascontiguousarray(lut, np.float32)
        _check(self._L.sgm_wls_filter_batch_device(self._h, n, arr(d_disps), arr(d_guides), int(cn), arr(d_confs), H, W, int(invalid),
                                                   float(lambda_), lut.ctypes.data, arr(d_outs), arr(d_out_f32s)))

    # -- the left-right consistency confidence (include/sgm_hip_lrc.h) --
    def lrc_confidence_host(self, disp_left: np.ndarray, disp_right: np.ndarray, base: np.ndarray | None, invalid: int, thresh: int,
                            radius: int, var_max: int, want_left: bool = True, want_right: bool = False):
        """sgm_lrc_confidence: int16 (H, W) left-view and right-view maps, uint8 (H, W) base confidence or None; returns
        (conf_left, conf_right), uint8 (H, W) each, None for the one that was not asked for."""
        disp_left = np.ascontiguousarray(disp_left, np.int16)
        disp_right = np.ascontiguousarray(disp_right, np.int16)
        base = None if base is None else np.ascontiguousarray(base, np.uint8)
        H, W = disp_left.shape
        cl = np.empty((H, W), np.uint8) if want_left else None
        cr = np.empty((H, W), np.uint8) if want_right else None
        _check(self._L.sgm_lrc_confidence(self._h, disp_left.ctypes.data, disp_right.ctypes.data,
                                          None if base is None else base.ctypes.data, H, W, int(invalid), int(thresh), int(radius),
                                          int(var_max), None if cl is None else cl.ctypes.data, None if cr is None else cr.ctypes.data))
        return cl, cr

    def lrc_confidence_device(self, d_left: int, d_right: int, d_base: int | None, H: int, W: int, invalid: int, thresh: int,
                              radius: int, var_max: int, d_conf_left: int | None, d_conf_right: int | None = None) -> None:
        """sgm_lrc_confidence_device: device addresses, in the order of the engine's stream."""
        _check(self._L.sgm_lrc_confidence_device(self._h, d_left, d_right, d_base, H, W, int(invalid), int(thresh), int(radius),
                                                 int(var_max), d_conf_left, d_conf_right))

    def lrc_confidence_batch_device(self, d_lefts, d_rights, d_bases, H: int, W: int, invalid: int, thresh: int, radius: int,
                                    var_max: int, d_conf_lefts, d_conf_rights=None) -> None:
        """sgm_lrc_confidence_batch_device: sequences of N device addresses (d_bases / d_conf_lefts / d_conf_rights: such a
        sequence, or None for none), in the order of the engine's stream."""
        n = len(d_lefts)
        arr = lambda xs: (C.c_void_p * len(xs))(*[int(x) if x else None for x in xs]) if xs is not None and len(xs) else None
        for xs in (d_rights, d_bases, d_conf_lefts, d_conf_rights):
            if xs is not None and len(xs) != n:
                raise error(f"lrc_confidence_batch_device: {n} pairs, but a sequence of {len(xs)} addresses")
        _check(self._L.sgm_lrc_confidence_batch_device(self._h, n, arr(d_lefts), arr(d_rights), arr(d_bases), H, W, int(invalid),
                                                       int(thresh), int(radius), int(var_max), arr(d_conf_lefts),
                                                       arr(d_conf_rights)))


# The notebook builds a matcher per call and throws it away (main.ipynb:655-668); engines are
# cached per (parameters, device) so device buffers survive between such calls.
_engine_cache: dict = {}
_CACHE_MAX = 4


def get_engine(params: dict, device: int | None = None) -> Engine:
    dev = get_device() if device is None else int(device)
    params = {**_DEFAULT, **params}
    key = (tuple(int(params[n]) for n in _PARAM_NAMES), dev)
    e = _engine_cache.get(key)
    if e is None:
        if len(_engine_cache) >= _CACHE_MAX:
            _engine_cache.pop(next(iter(_engine_cache)))
        e = Engine(params, dev)
        _engine_cache[key] = e
    return e


def clear_engine_cache() -> None:
    _engine_cache.clear()


@contextlib.contextmanager
def _option_for_this_call(eng: Engine, opt: int):
    """The cached engine produces the optional map (SGM_OPT_CONFIDENCE, SGM_OPT_RIGHT_VIEW) for this call only: plain
    compute() calls do not pay for it."""
    eng.set_option(opt, 1)
    try:
        yield
    finally:
        eng.set_option(opt, 0)


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


class StereoSGBM:
    """Mirror of cv2.StereoSGBM (the subset of the interface the reference exercises, plus the
    parameter getters/setters of the cv2 class)."""

    def __init__(self, costFunction=STEREO_COST_BT, **kw):
        self._p = {n: 0 for n in _PARAM_NAMES}
        self._p.update(numDisparities=16, blockSize=3)
        self.setCostFunction(costFunction)
        for k, v in kw.items():
            if k not in self._p:
                raise TypeError(f"StereoSGBM_create() got an unexpected keyword argument '{k}'")
            self._p[k] = int(v)

    # cv2-style accessors
    def __getattr__(self, name):
        if name.startswith(("get", "set")) and len(name) > 3:
            field = name[3].lower() + name[4:]
            field = {"mode": "mode", "p1": "P1", "p2": "P2"}.get(field, field)
            if field in self._p:
                if name.startswith("get"):
                    return lambda: self._p[field]
                return lambda v: self._p.__setitem__(field, int(v))
        raise AttributeError(name)

    def setCostFunction(self, costFunction):
        """STEREO_COST_BT (default) or STEREO_COST_CENSUS: the matching cost of this object's compute(),
        computeWithConfidence() and computeLeftRight() (SGM_OPT_COST, include/sgm_hip.h).  Census takes single-channel images."""
        if isinstance(costFunction, bool) or not isinstance(costFunction, (int, np.integer)) or \
                int(costFunction) not in (STEREO_COST_BT, STEREO_COST_CENSUS):
            raise error(f"StereoSGBM.setCostFunction: {costFunction!r} is neither STEREO_COST_BT (0) nor STEREO_COST_CENSUS (1)")
        self._cost = int(costFunction)

    def getCostFunction(self):
        return self._cost

    def _engine(self, cn: int, device: int | None = None) -> Engine:
        """The cached engine of these parameters, set to this object's cost function: the cache is keyed by the parameters
        alone and shared between matcher objects, so the option is set before EVERY compute, to 0 as well as to 1, and the
        callers set it back to STEREO_COST_BT behind the compute: other users of get_engine() (dist.py, pipeline.py) find the
        engine as they always did."""
        if self._cost == STEREO_COST_CENSUS and cn != 1:
            raise error("StereoSGBM.compute: STEREO_COST_CENSUS takes 8-bit single-channel (H, W) images; a colour census is not implemented")
        eng = get_engine(self._p, device)
        eng.set_option(_lib.SGM_OPT_COST, self._cost)
        return eng

    def compute(self, left, right):
        """int16 (H, W) disparity * 16, invalid = (minDisparity - 1) * 16  (main.ipynb:668).  left / right: uint8
        (H, W) or colour (H, W, 3) pairs of the same shape (the pixel cost sums the three channels, as cv2's)."""
        return self._compute(left, right, False)

    def computeWithConfidence(self, left, right):
        """(disp16, conf): compute()'s map and the per-pixel match confidence, uint8 (H, W) in 0 .. 100 -- the largest
        uniquenessRatio under which the winner-take-all would still keep the pixel ((far - minS) * 100 / far over the
        aggregated cost), 0 where the final disparity is invalid.  Same inputs and validation as compute(); numpy in,
        numpy out; HIP tensors in, tensors out.  Lets a consumer thin the point cloud after the fact
        (valid_points(..., confidence=conf, min_confidence=u)) instead of recomputing with another ratio.  No counterpart
        in cv2."""
        return self._compute(left, right, True)

    def computeLeftRight(self, left, right):
        """(disp16_left, disp16_right): compute()'s map and the disparity map referenced to the RIGHT image, int16 (H, W) at
        the same scale and with the same invalid value (minDisparity - 1) * 16; a valid right pixel (y, xr) with disparity d
        matches left pixel (y, xr + d).  Same inputs and validation as compute(); numpy in, numpy out; HIP tensors in, tensors
        out.  The right map comes from ONE more pass over the aggregated cost of this compute (right pixel xr at disparity d
        costs what left pixel xr + d paid for d), with the left map's uniqueness test, sub-pixel step, mirrored LR check,
        median and speckle filter -- not from a second compute.  It is NOT what cv2.ximgproc.createRightMatcher gives: that
        aggregates the paths again on the swapped pair; here they are the left view's."""
        return self._compute(left, right, False, True)

    def computeFiltered(self, left, right, lambda_=8000.0, sigmaColor=1.5, confidence="margin"):
        """A compute followed by the edge-aware filter (createDisparityWLSFilter) with `left` as the guide: int16 (H, W)
        disparity * 16 with the holes filled from confident neighbours, invalid (minDisparity - 1) * 16 only where no confidence
        reaches.  Colour pairs guide with all three channels.  numpy in, numpy out; HIP tensors in, a tensor out without leaving
        the device.  confidence says what weighs the filter:
          "margin"  (default) computeWithConfidence()'s uniqueness margin;
          "lrc"     the left-right consistency confidence (lrcConfidence, include/sgm_hip_lrc.h) of computeLeftRight()'s two
                    maps, with the filter's default threshold, radius and variance: one more pass over the aggregated cost;
          "both"    the same with the margin as its base: both optional maps of one compute."""
        _check_confidence_source(confidence)
        f = DisparityWLSFilter(self)
        f.setLambda(lambda_)
        f.setSigmaColor(sigmaColor)
        guide = left if _is_torch(left) else np.asarray(left)
        if len(guide.shape) == 3 and guide.shape[2] == 1:
            guide = guide[:, :, 0]
        if confidence == "margin":
            disp, conf = self.computeWithConfidence(left, right)
            return f.filter(disp, guide, conf)
        if confidence == "lrc":
            disp, rmap = self.computeLeftRight(left, right)
            return f.filter(disp, guide, None, disparity_map_right=rmap)
        disp, conf, rmap = self._compute(left, right, True, True)
        return f.filter(disp, guide, conf, disparity_map_right=rmap)

    def computeFilteredBatch(self, lefts, rights, lambda_=8000.0, sigmaColor=1.5, confidence="margin"):
        """computeFiltered() over N pairs of one shape: ONE batch compute with the confidence maps delivered per pair (the
        engine's sgm_pipeline_batch_device behind sgm_bind_confidence_device) and ONE batch filter call
        (sgm_wls_filter_batch_device) with `lefts` as the guides, both on the same engine.  confidence as in computeFiltered():
        "lrc" and "both" also bind the right-view maps in the same batch compute (sgm_bind_right_device) and put ONE batch
        confidence call (sgm_lrc_confidence_batch_device) between the compute and the filter, on the same engine and stream.  lefts / rights: uint8 stacks
        (N, H, W) or (N, H, W, 3), or sequences of N equal-shaped images; numpy (uploaded through torch, a numpy stack comes
        back) or HIP tensors (a tensor (N, H, W) comes back without leaving the device).  Result i equals
        computeFiltered(lefts[i], rights[i]) bit for bit.
        No synchronisation lies between the two calls: the batch compute leaves the engine's stream behind everything its
        internal engines did (run_group joins their streams into it; without a chained group the pairs run on that stream
        itself), and the filter is enqueued on the same stream."""
        _check_confidence_source(confidence)
        if self._p["mode"] not in (STEREO_SGBM_MODE_SGBM, STEREO_SGBM_MODE_HH, STEREO_SGBM_MODE_HH4):
            raise error("StereoSGBM.compute: MODE_SGBM, MODE_HH and MODE_HH4 are implemented; MODE_SGBM_3WAY is not "
                        "(its result depends on a stripe size upstream derives from the cache size)")
        f = DisparityWLSFilter(self)
        f.setLambda(lambda_)
        f.setSigmaColor(sigmaColor)
        L, R = _batch_items(lefts), _batch_items(rights)
        on_device = any(_is_torch(m) for m in L + R)
        if on_device:
            if not all(_is_torch(m) and m.is_cuda for m in L + R):
                raise error("StereoSGBM.computeFilteredBatch: torch inputs must all be CUDA (HIP) tensors")
            import torch
            u8 = torch.uint8
        else:
            L, R = [np.asarray(m) for m in L], [np.asarray(m) for m in R]
            u8 = np.uint8
        if len(L) == 0 or len(L) != len(R):
            raise error(f"StereoSGBM.computeFilteredBatch: {len(L)} left and {len(R)} right images (the same number, at least one)")
        shape = tuple(L[0].shape)
        if any(tuple(m.shape) != shape or m.dtype != u8 for m in L + R):
            raise error("StereoSGBM.compute: (-215:Assertion failed) left.size() == right.size() && "
                        "left.type() == right.type() && left.depth() == CV_8U")
        if len(shape) == 3 and shape[2] == 1:
            L, R, shape = [m[:, :, 0] for m in L], [m[:, :, 0] for m in R], shape[:2]
        _check_channels(len(shape), shape[2] if len(shape) == 3 else 1)
        if shape[0] == 0 or shape[1] == 0:
            raise error("StereoSGBM.compute: empty image")
        if shape[1] < 2:
            raise error("StereoSGBM.compute: image width < 2")
        import torch
        N, (H, W), cn = len(L), shape[:2], 1 if len(shape) == 2 else 3
        dev = L[0].device if on_device else torch.device("cuda", get_device())
        eng = self._engine(cn, dev.index or 0)      # (refuses a colour census before anything is uploaded)
        try:
            if not on_device:
                L = [torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in L]
                R = [torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in R]
            L, R = [m.contiguous() for m in L], [m.contiguous() for m in R]
            disp = torch.empty((N, H, W), dtype=torch.int16, device=dev)
            conf = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
            out = torch.empty((N, H, W), dtype=torch.int16, device=dev)
            ptrs = lambda ts: [t.data_ptr() for t in ts]
            # the engine runs on its own stream: order it after torch's current stream and wait for it (as _compute_torch does)
            torch.cuda.current_stream(dev).synchronize()
            if confidence == "margin":
                with _option_for_this_call(eng, _lib.SGM_OPT_CONFIDENCE):
                    eng.pipeline_batch_device(ptrs(L), ptrs(R), H, W, cn * W, None, ptrs(disp), cn=cn, d_confs=ptrs(conf))
            else:
                # conf receives the LR confidence; with "both" the margin goes to a stack of its own and is the base
                rmap = torch.empty((N, H, W), dtype=torch.int16, device=dev)
                base = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if confidence == "both" else None
                with contextlib.ExitStack() as on:
                    on.enter_context(_option_for_this_call(eng, _lib.SGM_OPT_RIGHT_VIEW))
                    if base is not None:
                        on.enter_context(_option_for_this_call(eng, _lib.SGM_OPT_CONFIDENCE))
                    eng.pipeline_batch_device(ptrs(L), ptrs(R), H, W, cn * W, None, ptrs(disp), cn=cn,
                                              d_confs=None if base is None else ptrs(base), d_rmaps=ptrs(rmap))
                eng.lrc_confidence_batch_device(ptrs(disp), ptrs(rmap), None if base is None else ptrs(base), H, W, f.defaultInvalid(),
                                                f.getLRCthresh(), f.getDepthDiscontinuityRadius(), f.getDiscontinuityVariance(),
                                                ptrs(conf))
            eng.wls_filter_batch_device(ptrs(disp), ptrs(L), cn, ptrs(conf), H, W, f.defaultInvalid(), lambda_, wls_weights(sigmaColor),
                                        ptrs(out))
            eng.synchronize()
        finally:
            eng.set_option(_lib.SGM_OPT_COST, STEREO_COST_BT)   # (as in _compute)
        return out if on_device else out.cpu().numpy()

    def _compute(self, left, right, with_conf: bool, with_right: bool = False):
        if self._p["mode"] not in (STEREO_SGBM_MODE_SGBM, STEREO_SGBM_MODE_HH, STEREO_SGBM_MODE_HH4):
            raise error("StereoSGBM.compute: MODE_SGBM, MODE_HH and MODE_HH4 are implemented; MODE_SGBM_3WAY is not "
                        "(its result depends on a stripe size upstream derives from the cache size)")
        if _is_torch(left) or _is_torch(right):
            return self._compute_torch(left, right, with_conf, with_right)
        left, right = np.asarray(left), np.asarray(right)
        # upstream: CV_Assert(left.size() == right.size() && left.type() == right.type() && depth == CV_8U)
        if left.shape != right.shape or left.dtype != right.dtype or left.dtype != np.uint8:
            raise error("StereoSGBM.compute: (-215:Assertion failed) left.size() == right.size() && "
                        "left.type() == right.type() && left.depth() == CV_8U")
        if left.ndim == 3 and left.shape[2] == 1:
            left, right = left[:, :, 0], right[:, :, 0]
        _check_channels(left.ndim, left.shape[2] if left.ndim == 3 else 1)
        if left.shape[0] == 0 or left.shape[1] == 0:
            raise error("StereoSGBM.compute: empty image")
        # pixels must be dense (a colour pixel is 3 adjacent bytes); padded rows pass as they are
        cn = 1 if left.ndim == 2 else 3
        px = (1,) if cn == 1 else (3, 1)
        if left.strides[1:] != px or left.strides[0] < cn * left.shape[1]:
            left = np.ascontiguousarray(left)
        if right.strides[1:] != px or right.strides[0] < cn * right.shape[1]:
            right = np.ascontiguousarray(right)
        if left.shape[1] < 2:
            raise error("StereoSGBM.compute: image width < 2")
        eng = self._engine(cn)
        try:
            if not (with_right or with_conf):
                return eng.compute_host(left, right)
            # one option: (disp, its map); both (computeFiltered's confidence="both"): (disp, conf, right)
            sides = ([(_lib.SGM_OPT_CONFIDENCE, _lib.SGM_TAP_CONF)] if with_conf else []) + \
                    ([(_lib.SGM_OPT_RIGHT_VIEW, _lib.SGM_TAP_RIGHT)] if with_right else [])
            with contextlib.ExitStack() as on:
                for opt, _ in sides:
                    on.enter_context(_option_for_this_call(eng, opt))
                disp = eng.compute_host(left, right)
                return (disp,) + tuple(eng.tap(tap, *disp.shape) for _, tap in sides)
        finally:
            eng.set_option(_lib.SGM_OPT_COST, STEREO_COST_BT)   # the cached engine goes back as get_engine() hands it out

    def _compute_torch(self, left, right, with_conf: bool = False, with_right: bool = False):
        import torch
        if not (_is_torch(left) and _is_torch(right)) or not left.is_cuda or not right.is_cuda:
            raise error("StereoSGBM.compute: torch inputs must both be CUDA (HIP) tensors")
        if left.shape != right.shape or left.dtype != torch.uint8 or right.dtype != torch.uint8:
            raise error("StereoSGBM.compute: (-215:Assertion failed) left.size() == right.size() && "
                        "left.type() == right.type() && left.depth() == CV_8U")
        if left.dim() == 3 and left.shape[2] == 1:
            left, right = left[:, :, 0], right[:, :, 0]
        _check_channels(left.dim(), left.shape[2] if left.dim() == 3 else 1)
        left, right = left.contiguous(), right.contiguous()
        H, W = left.shape[:2]
        cn = 1 if left.dim() == 2 else 3
        dev = left.device.index or 0
        eng = self._engine(cn, dev)
        try:
            out = torch.empty((H, W), dtype=torch.int16, device=left.device)
            # the engine runs on its own stream: order it after torch's current stream and wait for it
            torch.cuda.current_stream(left.device).synchronize()
            if not (with_right or with_conf):
                eng.compute_device(left.data_ptr(), right.data_ptr(), H, W, cn * W, out.data_ptr(), cn)
                eng.synchronize()
                return out
            sides, bound = [], {}
            with contextlib.ExitStack() as on:
                if with_conf:
                    sides.append(torch.empty((H, W), dtype=torch.uint8, device=left.device))
                    bound["d_conf"] = sides[-1].data_ptr()
                    on.enter_context(_option_for_this_call(eng, _lib.SGM_OPT_CONFIDENCE))
                if with_right:
                    sides.append(torch.empty((H, W), dtype=torch.int16, device=left.device))
                    bound["d_rmap"] = sides[-1].data_ptr()
                    on.enter_context(_option_for_this_call(eng, _lib.SGM_OPT_RIGHT_VIEW))
                eng.compute_device(left.data_ptr(), right.data_ptr(), H, W, cn * W, out.data_ptr(), cn, **bound)
                eng.synchronize()
        finally:
            eng.set_option(_lib.SGM_OPT_COST, STEREO_COST_BT)   # (as in _compute)
        return (out,) + tuple(sides)


def _batch_items(x) -> list:
    """the maps of a batch argument, one by one: the entries of a list or tuple, else the slices of a stack along its first axis"""
    if isinstance(x, (list, tuple)):
        return list(x)
    if not _is_torch(x):
        x = np.asarray(x)
    return [x[i] for i in range(x.shape[0])] if len(x.shape) >= 1 else [x]


def _check_channels(ndim: int, cn: int) -> None:
    """upstream: CV_Assert(cn == 1 || cn == 3) behind the size / type assertion -- 8-bit 1- or 3-channel pairs"""
    if ndim not in (2, 3) or (ndim == 3 and cn != 3):
        raise error("StereoSGBM.compute: (-215:Assertion failed) left.channels() == 1 || left.channels() == 3: "
                    "only 8-bit single-channel (H, W) and 3-channel (H, W, 3) images are supported")


def StereoSGBM_create(minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0,
                      preFilterCap=0, uniquenessRatio=0, speckleWindowSize=0, speckleRange=0,
                      mode=STEREO_SGBM_MODE_SGBM, costFunction=STEREO_COST_BT) -> StereoSGBM:
    """Same signature and defaults as cv2.StereoSGBM_create (OpenCV 4.11), and one trailing keyword of this package's own:
    costFunction, STEREO_COST_BT (default) or STEREO_COST_CENSUS (StereoSGBM.setCostFunction)."""
    return StereoSGBM(costFunction=costFunction, minDisparity=minDisparity, numDisparities=numDisparities, blockSize=blockSize, P1=P1, P2=P2,
                      disp12MaxDiff=disp12MaxDiff, preFilterCap=preFilterCap, uniquenessRatio=uniquenessRatio,
                      speckleWindowSize=speckleWindowSize, speckleRange=speckleRange, mode=mode)




_CONFIDENCE_SOURCES = ("margin", "lrc", "both")


def _check_confidence_source(confidence) -> None:
    if not isinstance(confidence, str) or confidence not in _CONFIDENCE_SOURCES:
        raise error(f"StereoSGBM.computeFiltered: confidence={confidence!r} is none of 'margin', 'lrc', 'both'")


LRC_THRESH_DEFAULT, LRC_RADIUS_DEFAULT, LRC_VAR_MAX_DEFAULT = 24, 5, 2304
LRC_RADIUS_MAX = 16


def _lrc_int(who: str, name: str, v, lo: int, hi: int) -> int:
    """an integer argument of the LR confidence inside its range (include/sgm_hip_lrc.h), or cv.error"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise error(f"{who}: {name}={v!r} is not an integer in {lo} .. {hi}")
    return int(v)


def _lrc_check_maps(who: str, dl, dr, base, i16, u8) -> None:
    """the right map (and base) against the left map: dtype, rank, shape"""
    if dl.dtype != i16 or dr.dtype != i16 or (base is not None and base.dtype != u8):
        raise error(f"{who}: (-215:Assertion failed) disparity_map_left.type() == CV_16SC1, disparity_map_right.type() == CV_16SC1, "
                    "confidence.type() == CV_8UC1")
    if len(dl.shape) != 2:
        raise error(f"{who}: the maps must be (H, W)")
    if tuple(dr.shape) != tuple(dl.shape) or (base is not None and tuple(base.shape) != tuple(dl.shape)):
        raise error(f"{who}: (-215:Assertion failed) the left map, the right map and the confidence must have the same size")
    if dl.shape[0] == 0 or dl.shape[1] == 0:
        raise error(f"{who}: empty image")


def lrcConfidence(disp_left, disp_right, base=None, invalid=-16, thresh=LRC_THRESH_DEFAULT, radius=LRC_RADIUS_DEFAULT,
                  var_max=LRC_VAR_MAX_DEFAULT, return_right=False):
    """The left-right consistency confidence (definition: include/sgm_hip_lrc.h): uint8 (H, W) in 0 .. 100 from the int16 maps of
    computeLeftRight() -- 0 where the two maps disagree by more than thresh sixteenths, where either is invalid and where the
    match leaves the image; elsewhere 100 minus the roughness of the maps inside a (2 radius + 1)^2 window against var_max
    (sixteenths squared), and no more than base (uint8 (H, W), computeWithConfidence's margin) when that is given.  Returns the
    left-view map, with return_right (left, right).  numpy in, numpy out; HIP tensors in, tensors out on the same device.
    This package's own definition in integers, NOT cv2's computeConfidenceMap bit for bit; cv2's ROI handling is not built."""
    who = "lrcConfidence"
    inv = _lrc_int(who, "invalid", invalid, -32768, 32767)
    T = _lrc_int(who, "thresh", thresh, 0, 32767)
    r = _lrc_int(who, "radius", radius, 0, LRC_RADIUS_MAX)
    V = _lrc_int(who, "var_max", var_max, 1, 1 << 30)
    maps = [disp_left, disp_right] + ([] if base is None else [base])
    if any(_is_torch(m) for m in maps):
        import torch
        if not all(_is_torch(m) and m.is_cuda for m in maps):
            raise error(f"{who}: torch inputs must all be CUDA (HIP) tensors")
        _lrc_check_maps(who, disp_left, disp_right, base, torch.int16, torch.uint8)
        dl, dr = disp_left.contiguous(), disp_right.contiguous()
        b = None if base is None else base.contiguous()
        H, W = int(dl.shape[0]), int(dl.shape[1])
        eng = get_engine(_DEFAULT, dl.device.index or 0)
        cl = torch.empty((H, W), dtype=torch.uint8, device=dl.device)
        cr = torch.empty((H, W), dtype=torch.uint8, device=dl.device) if return_right else None
        torch.cuda.current_stream(dl.device).synchronize()   # (as _compute_torch does)
        eng.lrc_confidence_device(dl.data_ptr(), dr.data_ptr(), None if b is None else b.data_ptr(), H, W, inv, T, r, V,
                                  cl.data_ptr(), None if cr is None else cr.data_ptr())
        eng.synchronize()
        return (cl, cr) if return_right else cl
    dl, dr = np.asarray(disp_left), np.asarray(disp_right)
    b = None if base is None else np.asarray(base)
    _lrc_check_maps(who, dl, dr, b, np.int16, np.uint8)
    cl, cr = get_engine(_DEFAULT).lrc_confidence_host(dl, dr, b, inv, T, r, V, True, bool(return_right))
    return (cl, cr) if return_right else cl


def wls_weights(sigma: float) -> np.ndarray:
    """The filter's default edge weights (sgm_wls_weights): float32 [256], exp(-k / sigma).  Needs no GPU."""
    lut = np.empty(256, np.float32)
    _check(_lib.load().sgm_wls_weights(float(sigma), lut.ctypes.data))
    return lut


class DisparityWLSFilter:
    """The place cv2.ximgproc.createDisparityWLSFilter takes in cv2 user code: a confidence-weighted, image-guided fast global
    smoother over a disparity map (definition: include/sgm_hip_wls.h).  It is this package's own definition, NOT cv2's filter
    bit for bit.  With a right-view map (filter(..., disparity_map_right=)) its weights are the left-right consistency
    confidence of include/sgm_hip_lrc.h, steered by setLRCthresh, setDepthDiscontinuityRadius and setDiscontinuityVariance and
    handed back by getConfidenceMap: the call shape of cv2's filter, a definition of our own in integers.  What remains
    unbuilt: cv2's ROI handling, and bit parity with cv2's filter and with its confidence map."""

    def __init__(self, matcher_left=None):
        self._matcher = matcher_left
        self._lambda = 8000.0
        self._sigma = 1.5
        self._lrc_thresh = LRC_THRESH_DEFAULT
        # cv2's default: ceil(0.5 * blockSize) of the matcher; 5 without one; capped to what the kernel's halo holds
        self._radius = min(LRC_RADIUS_MAX, (int(matcher_left.getBlockSize()) + 1) // 2) if matcher_left is not None else LRC_RADIUS_DEFAULT
        self._radius = max(0, self._radius)
        self._var_max = LRC_VAR_MAX_DEFAULT
        self._conf_map = None

    def setLRCthresh(self, thresh):
        """Largest difference of the two maps at a match, in sixteenths of a pixel (cv2: LRCthresh, default 24), 0 .. 32767"""
        self._lrc_thresh = _lrc_int("DisparityWLSFilter.setLRCthresh", "thresh", thresh, 0, 32767)

    def getLRCthresh(self):
        return self._lrc_thresh

    def setDepthDiscontinuityRadius(self, radius):
        """Half width of the window the roughness of the maps is measured in, 0 .. 16 pixels; 0 switches that factor off.
        Default: ceil(0.5 * blockSize) of the matcher, 5 without one, capped to 16."""
        self._radius = _lrc_int("DisparityWLSFilter.setDepthDiscontinuityRadius", "radius", radius, 0, LRC_RADIUS_MAX)

    def getDepthDiscontinuityRadius(self):
        return self._radius

    def setDiscontinuityVariance(self, var_max):
        """The variance inside the window, in sixteenths squared, at which the confidence reaches 0: 1 .. 2^30, default 2304
        (a standard deviation of three pixels).  No counterpart in cv2."""
        self._var_max = _lrc_int("DisparityWLSFilter.setDiscontinuityVariance", "var_max", var_max, 1, 1 << 30)

    def getDiscontinuityVariance(self):
        return self._var_max

    def getConfidenceMap(self):
        """The confidence the last filter() / filterBatch() call with a right-view map weighed the filter with: uint8 (H, W) in
        0 .. 100, a stack (N, H, W) after filterBatch; numpy or a HIP tensor, as that call's inputs were.  Raises before any
        such call.  (cv2 returns float32 in 0 .. 255, and another definition: include/sgm_hip_lrc.h.)"""
        if self._conf_map is None:
            raise error("DisparityWLSFilter.getConfidenceMap: no filter() call with disparity_map_right has been made")
        return self._conf_map

    def setLambda(self, lambda_):
        v = float(lambda_)
        if not (0.0 <= v <= 1e7):
            raise error(f"DisparityWLSFilter.setLambda: {lambda_!r} outside [0, 1e7]")
        self._lambda = v

    def getLambda(self):
        return self._lambda

    def setSigmaColor(self, sigma):
        v = float(sigma)
        if not (0.0 < v < float("inf")):
            raise error(f"DisparityWLSFilter.setSigmaColor: {sigma!r} is not a positive finite number")
        self._sigma = v

    def getSigmaColor(self):
        return self._sigma

    def defaultInvalid(self):
        """The value filter() takes for invalid pixels when it is given none: what the matcher's maps use"""
        return (int(self._matcher.getMinDisparity()) - 1) * 16 if self._matcher is not None else -16

    def _params(self):
        return self._matcher._p if self._matcher is not None else _DEFAULT

    def filter(self, disparity_map_left, left_view, confidence=None, invalid=None, return_float=False, disparity_map_right=None):
        """disparity_map_left: int16 (H, W), disparity * 16; left_view: the uint8 guide, (H, W) or (H, W, 3); confidence: uint8
        (H, W) in 0 .. 100 (computeWithConfidence's map) or None for full confidence on every valid pixel; invalid: the value
        that marks invalid pixels, by default (matcher_left.minDisparity - 1) * 16, -16 without a matcher.  Returns the filtered
        int16 map, with return_float (map, float32 disparity in pixels, 0 where invalid).  numpy in, numpy out; HIP tensors in,
        tensors out on the same device.
        disparity_map_right: the right-view map of computeLeftRight(), int16 (H, W), or None.  With it the filter is weighed
        with the left-right consistency confidence of the two maps (lrcConfidence with this object's LRCthresh,
        depthDiscontinuityRadius and discontinuity variance, `confidence` as its base), which getConfidenceMap() hands back.
        cv2 spells this call wls.filter(disp_left, left, None, disp_right)."""
        inv = self.defaultInvalid() if invalid is None else int(invalid)
        if not -32768 <= inv <= 32767:
            raise error(f"DisparityWLSFilter.filter: invalid value {inv} outside int16")
        maps = [disparity_map_left, left_view] + ([] if confidence is None else [confidence]) + \
               ([] if disparity_map_right is None else [disparity_map_right])
        on_device = any(_is_torch(m) for m in maps)
        if on_device:
            import torch
            if not all(_is_torch(m) and m.is_cuda for m in maps):
                raise error("DisparityWLSFilter.filter: torch inputs must all be CUDA (HIP) tensors")
            i16, u8 = torch.int16, torch.uint8
            d, g, c = disparity_map_left, left_view, confidence
        else:
            i16, u8 = np.int16, np.uint8
            d, g = np.asarray(disparity_map_left), np.asarray(left_view)
            c = None if confidence is None else np.asarray(confidence)
        if d.dtype != i16 or g.dtype != u8 or (c is not None and c.dtype != u8):
            raise error("DisparityWLSFilter.filter: (-215:Assertion failed) disparity_map_left.type() == CV_16SC1, "
                        "left_view.depth() == CV_8U, confidence.type() == CV_8UC1")
        if len(d.shape) != 2 or len(g.shape) not in (2, 3) or (len(g.shape) == 3 and g.shape[2] != 3):
            raise error("DisparityWLSFilter.filter: the map must be (H, W) and the guide (H, W) or (H, W, 3)")
        if tuple(g.shape[:2]) != tuple(d.shape) or (c is not None and tuple(c.shape) != tuple(d.shape)):
            raise error("DisparityWLSFilter.filter: (-215:Assertion failed) the map, the guide and the confidence must have the same size")
        H, W = int(d.shape[0]), int(d.shape[1])
        if H == 0 or W == 0:
            raise error("DisparityWLSFilter.filter: empty image")
        dr = None
        if disparity_map_right is not None:
            dr = disparity_map_right if on_device else np.asarray(disparity_map_right)
            _lrc_check_maps("DisparityWLSFilter.filter", d, dr, c, i16, u8)
        lut = wls_weights(self._sigma)
        cn = 1 if len(g.shape) == 2 else 3
        if not on_device:
            eng = get_engine(self._params())
            if dr is not None:
                c = eng.lrc_confidence_host(d, dr, c, inv, self._lrc_thresh, self._radius, self._var_max)[0]
                self._conf_map = c
            return eng.wls_filter_host(d, g, c, inv, self._lambda, lut, return_float)
        import torch
        d, g = d.contiguous(), g.contiguous()
        c = None if c is None else c.contiguous()
        eng = get_engine(self._params(), d.device.index or 0)
        out = torch.empty((H, W), dtype=torch.int16, device=d.device)
        outf = torch.empty((H, W), dtype=torch.float32, device=d.device) if return_float else None
        # the engine runs on its own stream: order it after torch's current stream and wait for it (as _compute_torch does)
        torch.cuda.current_stream(d.device).synchronize()
        if dr is not None:   # (both calls on the engine's stream, in order)
            dr, base = dr.contiguous(), c
            c = torch.empty((H, W), dtype=torch.uint8, device=d.device)
            eng.lrc_confidence_device(d.data_ptr(), dr.data_ptr(), None if base is None else base.data_ptr(), H, W, inv,
                                      self._lrc_thresh, self._radius, self._var_max, c.data_ptr())
            self._conf_map = c
        eng.wls_filter_device(d.data_ptr(), g.data_ptr(), cn, None if c is None else c.data_ptr(), H, W, inv, self._lambda, lut,
                              out.data_ptr(), None if outf is None else outf.data_ptr())
        eng.synchronize()
        return (out, outf) if return_float else out


    def filterBatch(self, disparity_maps, left_views, confidences=None, invalid=None, return_float=False, disparity_maps_right=None):
        """filter() over N maps of one shape in one engine call (sgm_wls_filter_batch): disparity_maps int16 (N, H, W), left_views
        uint8 (N, H, W) or (N, H, W, 3), confidences uint8 (N, H, W) or None -- stacks, or sequences of N equal-shaped maps;
        invalid and return_float as in filter().  numpy in, a numpy stack (N, H, W) out (with return_float: two); HIP tensors in
        (a stacked tensor or a sequence of tensors), a tensor (N, H, W) out without leaving the device.  Map i of the result
        equals filter() on map i alone, bit for bit.
        disparity_maps_right: the right-view maps, int16 (N, H, W) or a sequence, or None: as filter()'s disparity_map_right,
        map by map; getConfidenceMap() then hands back the stack (N, H, W) of the confidences."""
        inv = self.defaultInvalid() if invalid is None else int(invalid)
        if not -32768 <= inv <= 32767:
            raise error(f"DisparityWLSFilter.filter: invalid value {inv} outside int16")
        D, G = _batch_items(disparity_maps), _batch_items(left_views)
        Cf = None if confidences is None else _batch_items(confidences)
        Dr = None if disparity_maps_right is None else _batch_items(disparity_maps_right)
        maps = D + G + (Cf or []) + (Dr or [])
        on_device = any(_is_torch(m) for m in maps)
        if on_device:
            import torch
            if not all(_is_torch(m) and m.is_cuda for m in maps):
                raise error("DisparityWLSFilter.filter: torch inputs must all be CUDA (HIP) tensors")
            i16, u8 = torch.int16, torch.uint8
        else:
            i16, u8 = np.int16, np.uint8
            D, G = [np.asarray(m) for m in D], [np.asarray(m) for m in G]
            Cf = None if Cf is None else [np.asarray(m) for m in Cf]
            Dr = None if Dr is None else [np.asarray(m) for m in Dr]
        if any(m.dtype != i16 for m in D) or any(m.dtype != u8 for m in G + (Cf or [])):
            raise error("DisparityWLSFilter.filter: (-215:Assertion failed) disparity_map_left.type() == CV_16SC1, "
                        "left_view.depth() == CV_8U, confidence.type() == CV_8UC1")
        if len(D) == 0:
            raise error("DisparityWLSFilter.filterBatch: empty batch")
        if any(len(m.shape) != 2 for m in D) or any(len(m.shape) not in (2, 3) or (len(m.shape) == 3 and m.shape[2] != 3) for m in G):
            raise error("DisparityWLSFilter.filterBatch: the maps must be (N, H, W) and the guides (N, H, W) or (N, H, W, 3)")
        shape, gshape = tuple(D[0].shape), tuple(G[0].shape) if G else ()
        if len(G) != len(D) or (Cf is not None and len(Cf) != len(D)) or any(tuple(m.shape) != shape for m in D + (Cf or [])) or \
                any(tuple(m.shape) != gshape for m in G) or gshape[:2] != shape:
            raise error("DisparityWLSFilter.filter: (-215:Assertion failed) the map, the guide and the confidence must have the same size")
        N, (H, W) = len(D), shape
        if H == 0 or W == 0:
            raise error("DisparityWLSFilter.filter: empty image")
        if Dr is not None:
            if len(Dr) != N:
                raise error("DisparityWLSFilter.filter: (-215:Assertion failed) the left map, the right map and the confidence must "
                            "have the same size")
            for i in range(N):
                _lrc_check_maps("DisparityWLSFilter.filter", D[i], Dr[i], None, i16, u8)
        lut = wls_weights(self._sigma)
        cn = 1 if len(gshape) == 2 else 3
        if not on_device:
            stack = lambda x, items: np.ascontiguousarray(x) if isinstance(x, np.ndarray) else np.stack(items)
            eng = get_engine(self._params())
            confs = None if Cf is None else stack(confidences, Cf)
            if Dr is not None:   # (host maps: the confidence map by map through the host entry, then one batch filter call)
                confs = np.stack([eng.lrc_confidence_host(D[i], Dr[i], None if Cf is None else Cf[i], inv, self._lrc_thresh,
                                                          self._radius, self._var_max)[0] for i in range(N)])
                self._conf_map = confs
            return eng.wls_filter_batch_host(stack(disparity_maps, D), stack(left_views, G), confs, inv, self._lambda, lut, return_float)
        import torch
        D, G = [m.contiguous() for m in D], [m.contiguous() for m in G]
        Cf = None if Cf is None else [m.contiguous() for m in Cf]
        dev = D[0].device
        eng = get_engine(self._params(), dev.index or 0)
        out = torch.empty((N, H, W), dtype=torch.int16, device=dev)
        outf = torch.empty((N, H, W), dtype=torch.float32, device=dev) if return_float else None
        ptrs = lambda ts: None if ts is None else [t.data_ptr() for t in ts]
        # the engine runs on its own stream: order it after torch's current stream and wait for it (as filter() does)
        torch.cuda.current_stream(dev).synchronize()
        if Dr is not None:   # (both batch calls on the engine's stream, in order, nothing in between)
            Dr = [m.contiguous() for m in Dr]
            confs = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
            eng.lrc_confidence_batch_device(ptrs(D), ptrs(Dr), ptrs(Cf), H, W, inv, self._lrc_thresh, self._radius, self._var_max,
                                            ptrs(confs))
            self._conf_map = confs
            Cf = confs
        eng.wls_filter_batch_device(ptrs(D), ptrs(G), cn, ptrs(Cf), H, W, inv, self._lambda, lut, ptrs(out), ptrs(outf))
        eng.synchronize()
        return (out, outf) if return_float else out


def createDisparityWLSFilter(matcher_left=None) -> DisparityWLSFilter:
    """Call shape of cv2.ximgproc.createDisparityWLSFilter(matcher_left); see DisparityWLSFilter for what differs."""
    return DisparityWLSFilter(matcher_left)


def reprojectImageTo3D(disparity, Q, _3dImage=None, handleMissingValues=False, ddepth=-1):
    """float32 (H, W, 3) = Q . [x, y, d, 1] / W   (main.ipynb:697)."""
    if ddepth not in (-1, CV_32F):
        raise error("reprojectImageTo3D: only ddepth=-1 / CV_32F is implemented (the reference uses the default)")
    Q = np.asarray(Q)
    if Q.shape != (4, 4):
        raise error("reprojectImageTo3D: (-215:Assertion failed) Q.size() == Size(4,4)")
    Q = np.ascontiguousarray(Q, np.float64)
    if _is_torch(disparity):
        import torch
        if not disparity.is_cuda or disparity.dim() != 2:
            raise error("reprojectImageTo3D: torch disparity must be a 2-D CUDA tensor")
        d = disparity.to(torch.float32).contiguous()
        H, W = d.shape
        eng = get_engine(_DEFAULT, d.device.index or 0)
        out = torch.empty((H, W, 3), dtype=torch.float32, device=d.device)
        torch.cuda.current_stream(d.device).synchronize()
        eng.reproject_device(d.data_ptr(), H, W, Q, bool(handleMissingValues), out.data_ptr())
        eng.synchronize()
        return out
    d = np.asarray(disparity)
    # upstream accepts CV_8UC1, CV_16SC1, CV_32SC1, CV_32FC1 and converts each row to float
    if d.ndim != 2 or d.dtype not in (np.uint8, np.int16, np.int32, np.float32):
        raise error("reprojectImageTo3D: (-215:Assertion failed) stype == CV_8UC1 || stype == CV_16SC1 || "
                    "stype == CV_32SC1 || stype == CV_32FC1")
    if d.size == 0:
        raise error("reprojectImageTo3D: empty disparity")
    d = np.ascontiguousarray(d, np.float32)
    return get_engine(_DEFAULT).reproject_host(d, Q, bool(handleMissingValues))


# ---- rectification in front of the path (gui.py:160-164, main.ipynb cell 7) ----
CV_32FC1 = 5
CV_16SC2 = 11
INTER_NEAREST, INTER_LINEAR, INTER_CUBIC = 0, 1, 2
BORDER_CONSTANT = 0


def initUndistortRectifyMap(cameraMatrix, distCoeffs, R, newCameraMatrix, size, m1type, map1=None, map2=None):
    """(map1, map2) float32 (H, W) source coordinates for every destination pixel
    (cv2.initUndistortRectifyMap(K0, None, R1, P1, image_size, cv2.CV_32F), gui.py:160)."""
    if m1type not in (CV_32F, CV_32FC1):
        raise error("initUndistortRectifyMap: only m1type=CV_32FC1 (two float maps, what the reference asks for) is implemented")
    W, H = int(size[0]), int(size[1])
    if W <= 0 or H <= 0:
        raise error("initUndistortRectifyMap: (-215:Assertion failed) size.width > 0 && size.height > 0")
    K = np.asarray(cameraMatrix)
    if K.shape != (3, 3):
        raise error("initUndistortRectifyMap: (-215:Assertion failed) A.size() == Size(3,3)")
    if distCoeffs is not None and np.asarray(distCoeffs).size == 0:
        distCoeffs = None
    if distCoeffs is not None and np.asarray(distCoeffs).size not in (4, 5, 8, 12, 14):
        raise error("initUndistortRectifyMap: (-215:Assertion failed) distCoeffs must hold 4, 5, 8, 12 or 14 values")
    if R is not None and np.asarray(R).size == 0:
        R = None
    if R is not None and np.asarray(R).shape != (3, 3):
        raise error("initUndistortRectifyMap: (-215:Assertion failed) R.size() == Size(3,3)")
    if newCameraMatrix is not None and np.asarray(newCameraMatrix).size == 0:
        newCameraMatrix = None
    return get_engine(_DEFAULT).init_undistort_rectify_map_host(K, distCoeffs, R, newCameraMatrix, W, H)


def remap(src, map1, map2, interpolation, dst=None, borderMode=BORDER_CONSTANT, borderValue=0):
    """Bilinear gather of an 8-bit image through a float map pair
    (cv2.remap(imgL, mapL1, mapL2, interpolation=cv2.INTER_LINEAR), gui.py:163)."""
    if interpolation != INTER_LINEAR:
        raise error("remap: only interpolation=INTER_LINEAR (what the reference uses) is implemented")
    if borderMode != BORDER_CONSTANT or np.any(np.asarray(borderValue) != 0):
        raise error("remap: only borderMode=BORDER_CONSTANT with borderValue=0 (the defaults) is implemented")
    s = np.asarray(src)
    if s.dtype != np.uint8 or s.ndim not in (2, 3) or (s.ndim == 3 and not 1 <= s.shape[2] <= 4) or s.size == 0:
        raise error("remap: source must be a non-empty uint8 image with 1..4 channels")
    m1, m2 = np.asarray(map1), np.asarray(map2)
    if m1.dtype != np.float32 or m2.dtype != np.float32 or m1.ndim != 2 or m1.shape != m2.shape or m1.size == 0:
        raise error("remap: (-215:Assertion failed) map1 and map2 must be CV_32FC1 of the same size")
    s = np.ascontiguousarray(s)
    return get_engine(_DEFAULT).remap_linear_host(s, np.ascontiguousarray(m1), np.ascontiguousarray(m2))
