"""The stage record of every add-on call, stage by stage: with SGM_OPT_PROFILE on, Engine.stage_times() after one call is
exactly the (name, launches) sequence written here.  The tables are the record of the engine as it stood before its add-ons went
through run_stage and one host staging call; a change of the engine's plumbing must leave every one of them as it is."""
import numpy as np
import pytest

from stereo_reconstruction_cv_amd import _lib
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu

R = 0.2                   # the search radius: about ten neighbours per point of the cube
ORG = (0.0, 0.0, 0.0)
FAR = 1e7                 # a finite coordinate no cell of a grid of R (or of voxels of R) reaches
H, W = 6, 8


def cube(stray: bool) -> np.ndarray:
    """300 points in the unit cube; stray: and five that are not finite or lie in no cell"""
    xyz = np.random.default_rng(7).random((300, 3), dtype=np.float32)
    if stray:
        nan, inf = np.nan, np.inf
        xyz = np.concatenate([xyz, np.array([[nan, .5, .5], [.5, inf, .5], [FAR, .5, .5], [.5, .5, -FAR], [nan, nan, nan]], np.float32)])
    return xyz


def nowhere() -> np.ndarray:
    """a cloud with no point in range"""
    return np.array([[FAR, 0, 0], [0, -FAR, 0], [np.nan, 0, 0], [0, 0, FAR]], np.float32)


def organised():
    """a 6 x 8 cloud on a tilted plane, three of its disparities invalid"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    xyz = np.stack([x, y, 10 + 0.1 * x + 0.05 * y], axis=2).astype(np.float32)
    disp = np.full((H, W), 4.0, np.float32)
    disp[0, 0], disp[2, 5], disp[5, 7] = 0.0, -1.0, 0.0
    return xyz, disp


class Dev:
    """device memory for one call: up(array) and room(shape, dtype) give addresses, the tensors live as long as this does"""

    def __init__(self, e):
        import torch
        self.torch, self.dev, self.held = torch, torch.device("cuda", e.device), []

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.held.append(t)
        return t.data_ptr()

    def room(self, shape, dtype):
        t = self.torch.zeros(shape, dtype=getattr(self.torch, dtype), device=self.dev)
        self.held.append(t)
        return t.data_ptr()

    def ready(self):
        self.torch.cuda.synchronize()


def radius(e, d, rows, xyz=None):
    xyz = cube(True) if xyz is None else xyz
    n = len(xyz)
    px = d.up(xyz)
    keep, pts = d.room(n, "uint8"), d.room((n, 3), "float32") if rows else None
    d.ready()
    e.radius_outlier_device(px, None, None, n, R, 4, None, ORG, keep, None, pts)


def statistical(e, d, rows):
    xyz = cube(True)
    n = len(xyz)
    px = d.up(xyz)
    keep, idx = d.room(n, "uint8"), d.room(n, "int32") if rows else None
    d.ready()
    e.statistical_outlier_device(px, None, None, n, 8, 1.0, R, ORG, keep, None, None, None, idx)


def covariance(e, d, stray, debug=0):
    xyz = cube(stray)
    n = len(xyz)
    px, nrm = d.up(xyz), d.room((n, 3), "float32")
    d.ready()
    e.set_option(_lib.SGM_OPT_DEBUG, debug)
    try:
        stats = e.covariance_normals_device(px, None, n, R, 3, ORG, ORG, True, nrm)
    finally:
        e.set_option(_lib.SGM_OPT_DEBUG, 0)
    assert int(stats[0]) == 300 and (int(stats[0]) < n) == stray   # the fill launch runs exactly when a point is in no cell


def dbscan(e, d):
    xyz = cube(True)
    n = len(xyz)
    px, lab = d.up(xyz), d.room(n, "int32")
    d.ready()
    e.cluster_dbscan_device(px, None, n, R, 4, ORG, lab)


def voxel(e, d):
    xyz = cube(True)
    n = len(xyz)
    px, pts = d.up(xyz), d.room((n, 3), "float32")
    d.ready()
    e.voxel_downsample_device(px, None, None, n, R, ORG, 1, pts)


def plane(e, d, refine, rows):
    xyz = cube(True)
    n = len(xyz)
    px, inl = d.up(xyz), d.room(n, "uint8")
    pts = d.room((n, 3), "float32") if rows else None
    d.ready()
    e.segment_plane_device(px, None, None, n, 0.05, 64, 1, refine, 0, inl, None, pts)


def plane_inliers(e, d, rows):
    xyz = cube(True)
    n = len(xyz)
    px, inl = d.up(xyz), d.room(n, "uint8")
    pts = d.room((n, 3), "float32") if rows else None
    d.ready()
    e.plane_inliers_device(px, None, None, n, (0.0, 0.0, 1.0, -0.5), 0.05, 0, inl, None, pts)


def mesh(e, d, normals):
    xyz, disp = organised()
    px, pd = d.up(xyz), d.up(disp)
    vert, faces = d.room((H * W, 3), "float32"), d.room((2 * (H - 1) * (W - 1), 3), "int32")
    nrm = d.room((H * W, 3), "float32") if normals else None
    d.ready()
    if normals:
        e.mesh_grid_normals_device(px, pd, None, H, W, 1.0, True, vert, None, faces, nrm)
    else:
        e.mesh_grid_device(px, pd, None, H, W, 1.0, vert, None, faces)


def normals_grid(e, d):
    xyz, disp = organised()
    px, pd, nrm = d.up(xyz), d.up(disp), d.room((H * W, 3), "float32")
    d.ready()
    e.normals_grid_device(px, pd, H, W, 1.0, True, nrm)


def icp(e, d):
    tgt = cube(True)
    src = (cube(False) + np.float32(0.01)).astype(np.float32)
    ps, pt = d.up(src), d.up(tgt)
    d.ready()
    stats = e.register_icp_device(ps, None, len(src), pt, None, None, len(tgt), R, ORG, None, 0, 2, 0.0, 0.0)[4]
    assert int(stats[3]) == 2, stats   # two iterations: three evaluations, of which the record keeps the last


SEP = _lib.SGM_DBG_COV_SEPARATE_SOLVE
CASES = {
    "radius_rows": (lambda e, d: radius(e, d, True),
                    [("radius_count", 1), ("radius_clear", 1), ("radius_insert", 1), ("radius_starts", 1), ("radius_sort", 1),
                     ("radius_query", 1), ("radius_compact", 3)]),
    "radius_no_rows": (lambda e, d: radius(e, d, False),
                       [("radius_count", 1), ("radius_clear", 1), ("radius_insert", 1), ("radius_starts", 1), ("radius_sort", 1),
                        ("radius_query", 1), ("radius_compact", 2)]),
    "radius_nothing_in_range": (lambda e, d: radius(e, d, True, nowhere()), [("radius_count", 1)]),
    "statistical_rows": (lambda e, d: statistical(e, d, True),
                         [("stat_count", 1), ("stat_clear", 1), ("stat_insert", 1), ("stat_starts", 1), ("stat_sort", 1),
                          ("stat_query", 1), ("stat_reduce", 1), ("stat_keep", 1), ("stat_compact", 3)]),
    "statistical_no_rows": (lambda e, d: statistical(e, d, False),
                            [("stat_count", 1), ("stat_clear", 1), ("stat_insert", 1), ("stat_starts", 1), ("stat_sort", 1),
                             ("stat_query", 1), ("stat_reduce", 1), ("stat_keep", 1), ("stat_compact", 2)]),
    "covariance_with_invalid": (lambda e, d: covariance(e, d, True),
                                [("cov_count", 1), ("cov_clear", 1), ("cov_insert", 1), ("cov_starts", 1), ("cov_sort", 1),
                                 ("cov_query", 2)]),
    "covariance_all_valid": (lambda e, d: covariance(e, d, False),
                             [("cov_count", 1), ("cov_clear", 1), ("cov_insert", 1), ("cov_starts", 1), ("cov_sort", 1),
                              ("cov_query", 1)]),
    "covariance_separate_solve": (lambda e, d: covariance(e, d, True, SEP),
                                  [("cov_count", 1), ("cov_clear", 1), ("cov_insert", 1), ("cov_starts", 1), ("cov_sort", 1),
                                   ("cov_query", 2), ("cov_solve", 1)]),
    "dbscan": (dbscan,
               [("dbscan_count", 1), ("dbscan_clear", 1), ("dbscan_insert", 1), ("dbscan_starts", 1), ("dbscan_sort", 1),
                ("dbscan_core", 2), ("dbscan_link", 1), ("dbscan_number", 3), ("dbscan_label", 1)]),
    "voxel": (voxel, [("voxel_count", 1), ("voxel_clear", 1), ("voxel_insert", 1), ("voxel_heads", 3)]),
    "plane_refine_rows": (lambda e, d: plane(e, d, True, True),
                          [("plane_valid", 3), ("plane_sample", 1), ("plane_count", 1), ("plane_best", 1), ("plane_moments", 1),
                           ("plane_solve", 1), ("plane_classify", 1), ("plane_compact", 3)]),
    "plane_no_refine_no_rows": (lambda e, d: plane(e, d, False, False),
                                [("plane_valid", 3), ("plane_sample", 1), ("plane_count", 1), ("plane_best", 1),
                                 ("plane_classify", 1), ("plane_compact", 2)]),
    "plane_inliers_rows": (lambda e, d: plane_inliers(e, d, True), [("plane_classify", 1), ("plane_compact", 3)]),
    "plane_inliers_no_rows": (lambda e, d: plane_inliers(e, d, False), [("plane_classify", 1), ("plane_compact", 2)]),
    "mesh": (lambda e, d: mesh(e, d, False),
             [("mesh_quads", 1), ("mesh_used", 1), ("mesh_scan", 2), ("mesh_vertices", 1), ("mesh_faces", 1)]),
    "mesh_normals": (lambda e, d: mesh(e, d, True),
                     [("mesh_quads", 1), ("mesh_used", 1), ("mesh_scan", 2), ("mesh_vertices", 1), ("mesh_faces", 1),
                      ("mesh_normals", 1)]),
    "normals_grid": (normals_grid, [("mesh_quads", 1), ("normals_grid", 1)]),
    "icp_two_iterations": (icp,
                           [("icp_count", 1), ("icp_clear", 1), ("icp_insert", 1), ("icp_starts", 1), ("icp_sort", 1),
                            ("icp_correspond", 1), ("icp_terms", 1), ("icp_reduce", 1)]),
}


@pytest.fixture(scope="module")
def eng():
    e = Engine({"numDisparities": 16})
    e.set_option(_lib.SGM_OPT_PROFILE, 1)
    return e


@pytest.mark.parametrize("case", list(CASES))
def test_the_stage_record_of_the_call(eng, case):
    call, want = CASES[case]
    call(eng, Dev(eng))
    got = [(name, launches) for name, ms, launches in eng.stage_times()]
    assert got == want + [("_wall", 0)], got
