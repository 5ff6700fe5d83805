"""Voxel-grid downsampling without a GPU: hand-worked answers of the definition (include/sgm_hip_voxel.h) held against its numpy
restatement tests/voxel_ref.py, the reference's independence of the order of the points, the accuracy of the definition against
the exact mean, the condition on the generated clouds that keeps the device tests from passing on trivial input, the interface
lists (header, binding, library, ABI version) and the Python argument errors, all of which are raised before any engine exists.
What the device computes is held against voxel_ref.py in tests/test_gpu_voxel.py."""
import os
import re

import numpy as np
import pytest

import voxel_ref as VR
import stereo_reconstruction_cv_amd as cv
from stereo_reconstruction_cv_amd import _lib
from stereo_reconstruction_cv_amd import stereo as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sgm_voxel_downsample", "sgm_voxel_downsample_device"]
F32 = np.float32


def f32(x):
    return np.asarray(x, np.float32)


def run(xyz, disp=None, colors=None, v=1.0, origin=(0, 0, 0), min_points=1):
    return VR.voxel_downsample(f32(xyz).reshape(-1, 3), None if disp is None else f32(disp),
                               None if colors is None else np.asarray(colors, np.uint8).reshape(-1, 3), v, origin, min_points)


# ---- the definition, by hand -----------------------------------------------------------------------------------------------------
def test_two_points_in_one_voxel_by_hand():
    """v = 1: (0.25, 0.5, 0.75) and (0.75, 0.5, 0.25) share voxel (0, 0, 0).  u = 16384 / 32768 / 49152 and 49152 / 32768 / 16384,
    S = 65536 on every axis, c = 2, M = (131072 + 2) / 4 = 32768, m = 0.5: the centroid is (0.5, 0.5, 0.5)"""
    r = run([[0.25, 0.5, 0.75], [0.75, 0.5, 0.25]], colors=[[10, 20, 30], [20, 40, 60]])
    assert (2 * 65536 + 2) // 4 == 32768
    assert r["n_voxels"] == 1 and r["n_out_of_range"] == 0
    assert r["points"].tolist() == [[0.5, 0.5, 0.5]] and r["counts"].tolist() == [2]
    assert r["colors"].tolist() == [[15, 30, 45]]
    assert r["keys"].tolist() == [(1 << 20) << 42 | (1 << 20) << 21 | (1 << 20)] and r["first"].tolist() == [0]


def test_round_half_up_of_the_mean_fraction_and_of_the_colour():
    """u = 1 and u = 2 (x = 1/65536 and 2/65536, exact in binary32): S = 3, c = 2, M = (6 + 2) / 4 = 2 -- 1.5 rounds UP; colours
    10 and 11: (42 + 2) / 4 = 11 -- 10.5 rounds up; 10, 10, 11: (62 + 3) / 6 = 10 -- 10.33 rounds down"""
    a, b = 1.0 / 65536, 2.0 / 65536
    r = run([[a, 0, 0], [b, 0, 0]], colors=[[10, 0, 255], [11, 0, 255]])
    assert r["points"][0, 0] == F32(2.0 / 65536) and r["colors"].tolist() == [[11, 0, 255]]
    r = run([[a, 0, 0], [a, 0, 0], [b, 0, 0]], colors=[[10, 1, 0], [10, 1, 0], [11, 2, 0]])
    assert (2 * 4 + 3) // 6 == 1 and (2 * 31 + 3) // 6 == 10 and (2 * 4 + 3) // 6 == 1
    assert r["points"][0, 0] == F32(1.0 / 65536) and r["colors"].tolist() == [[10, 1, 0]] and r["counts"].tolist() == [3]


def test_the_saturation_of_a_tiny_negative_coordinate():
    """t = -1e-10: g = -1 and t - g rounds to exactly 1.0f, so u is capped at 65535 and the centroid is -1/65536 of a voxel"""
    t = F32(-1e-10)
    assert np.floor(t) == -1 and t - np.floor(t) == F32(1.0)
    for v in (1.0, 0.05):
        r = run([[-1e-10, 0, 0]], v=v)
        want = (F32(-1) + F32(65535) * F32(1.0 / 65536)) * F32(v)
        assert want == F32(-1.0 / 65536) * F32(v)
        assert r["points"][0].tolist() == [want, 0.0, 0.0] and r["n_voxels"] == 1
        assert (r["keys"][0] >> 42) == (1 << 20) - 1


def test_the_last_index_is_kept_and_the_next_is_counted_out():
    """v = 1: x = 2^20 - 0.5 has g = 2^20 - 1 (kept), x = 2^20 has g = 2^20 (out of range, counted), -2^20 is kept,
    -2^20 - 1 is out; an out-of-range index on ONE axis is enough"""
    top = float(2 ** 20)
    r = run([[top - 0.5, 0, 0], [top, 0, 0], [-top, 0, 0], [-top - 1, 0, 0], [0, 0, top], [0, 3e38, 0]])
    assert r["n_voxels"] == 2 and r["n_out_of_range"] == 4
    assert r["points"].tolist() == [[top - 0.5, 0, 0], [-top, 0, 0]]
    assert (r["keys"] >> 42).tolist() == [2 ** 21 - 1, 0]


def test_nan_in_one_coordinate_alone_and_nonpositive_disparities():
    """the compaction looks at X alone; here NaN or inf in ANY coordinate makes a point invalid (not out of range), and so does
    disp <= 0 or a NaN disparity"""
    pts = [[0.5, np.nan, 0.5], [0.5, 0.5, np.inf], [-np.inf, 0.5, 0.5], [0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [3.5, 0.5, 0.5]]
    r = run(pts)
    assert r["n_voxels"] == 4 and r["n_out_of_range"] == 0 and r["first"].tolist() == [3, 4, 5, 6]
    r = run(pts, disp=[1, 1, 1, 0.0, -2.0, np.nan, 0.25])
    assert r["n_voxels"] == 1 and r["first"].tolist() == [6] and r["n_out_of_range"] == 0
    r = run([[np.nan] * 3] * 5)
    assert r["n_voxels"] == 0 and r["points"].shape == (0, 3) and r["counts"].shape == (0,)


def test_a_nonzero_origin_moves_the_grid():
    """v = 0.5, o = (0.25, 0, -1): x = 0.3 sits in the voxel [0.25, 0.75) whatever the grid at the origin would say"""
    r = run([[0.3, 0.1, -0.9], [0.7, 0.4, -0.6], [0.8, 0.1, -0.9]], v=0.5, origin=(0.25, 0, -1))
    assert r["n_voxels"] == 2 and r["counts"].tolist() == [2, 1]
    t = (f32([0.3, 0.7]) - F32(0.25)) * F32(2.0)
    u = (t * F32(65536)).astype(np.int64)
    M = (2 * int(u.sum()) + 2) // 4
    assert r["points"][0, 0] == (F32(0) + F32(M) * F32(1 / 65536)) * F32(0.5) + F32(0.25)
    assert abs(float(r["points"][0, 0]) - 0.5) < 1e-5 and abs(float(r["points"][0, 2]) + 0.75) < 1e-5


def test_min_points_keeps_the_order_of_the_first_points():
    """voxels A (x = 0..1), B, C, D, E visited as B A C A B D B A E A A: counts A 5, B 3, C 1, D 1, E 1; firsts B 0, A 1, C 2, D 5, E 8"""
    xs = dict(A=0.5, B=1.5, C=2.5, D=3.5, E=4.5)
    seq = "BACABDBAEAA"
    pts = [[xs[s], 0.5, 0.5] for s in seq]
    r1, r2, r5 = (run(pts, min_points=k) for k in (1, 2, 5))
    assert r1["first"].tolist() == [0, 1, 2, 5, 8] and r1["counts"].tolist() == [3, 5, 1, 1, 1]
    assert r2["first"].tolist() == [0, 1] and r2["counts"].tolist() == [3, 5] and r2["points"][:, 0].tolist() == [1.5, 0.5]
    assert r5["first"].tolist() == [1] and r5["counts"].tolist() == [5]
    assert run(pts, min_points=6)["n_voxels"] == 0


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
def test_the_reference_does_not_depend_on_the_order_of_the_points():
    xyz, disp, col = VR.layered_cloud(48, 320, 11)
    xyz, disp, col = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)
    a = VR.voxel_downsample(xyz, disp, col, 0.05)
    perm = np.random.default_rng(5).permutation(xyz.shape[0])
    b = VR.voxel_downsample(xyz[perm], disp[perm], col[perm], 0.05)
    assert a["n_voxels"] == b["n_voxels"] > 500 and a["n_out_of_range"] == b["n_out_of_range"]
    ia, ib = np.argsort(a["keys"]), np.argsort(b["keys"])
    assert np.array_equal(a["keys"][ia], b["keys"][ib])
    for k in ("points", "colors", "counts"):
        assert np.array_equal(a[k][ia], b[k][ib]), k
    # first is an index into the caller's order, and the output is in ascending order of it
    assert (np.diff(a["first"]) > 0).all() and (np.diff(b["first"]) > 0).all()
    assert np.array_equal(VR.keys_of(VR.classify(xyz[perm], disp[perm], 0.05, (0, 0, 0))[2][b["first"]]), b["keys"])


def test_the_centroid_stays_within_the_derived_bound_of_the_exact_mean():
    """Bound, per coordinate, against the float64 mean p_bar of a voxel's members, with R = max(|p|, |o|, |centroid|) over the
    voxel and eps = 2^-24 (half an ulp, relative, of binary32 round-to-nearest):
      * t = (p - o) * inv: p - o rounds with at most eps * 2R absolute error, the product adds eps relative of |t| v <= 2R, and
        inv = fl(1 / v) is off by eps relative, which moves t * v by at most eps * 2R: 3 roundings, each <= 2 eps R in units of
        length.  f = t - g is exact (g is t's integer part and |f| <= 1 needs no more bits than t has).
      * u = floor(65536 f) is below 65536 f by less than 1, so the mean of u / 65536 is below the mean of f by less than 2^-16
        of a voxel; M rounds that mean to the nearest 1/65536: another 2^-17.  Together less than v * 2^-15.
      * step 6: g + m, * v, + o are three roundings of values of magnitude <= 2R (+ o: <= R): <= 2 eps R each.
    Total: v * 2^-15 + 6 * 2 eps R = v * 2^-15 + 12 * 2^-24 R, i.e. 12 half-ulps -- 6 binary32 ulps -- of max(|p|, |o|).  At
    v = 0.05 the first term is 1.5e-6; with R about 3 the second is 2.1e-6."""
    eps = 2.0 ** -24
    worst = 0.0
    for seed, v, o in ((21, 0.05, (0.0, 0.0, 0.0)), (22, 0.05, (-0.5, 0.25, 1.0)), (23, 0.011, (0.0, 0.0, 0.0))):
        xyz, disp, col = VR.layered_cloud(48, 320, seed)
        xyz, disp = xyz.reshape(-1, 3), disp.reshape(-1)
        r = VR.voxel_downsample(xyz, disp, None, v, o)
        valid, inr, g, u = VR.classify(xyz, disp, v, o)
        idx = np.nonzero(inr)[0]
        key = VR.keys_of(g[idx])
        order = {int(k): j for j, k in enumerate(r["keys"])}
        row = np.array([order[int(k)] for k in key])
        s = np.zeros((r["n_voxels"], 3))
        np.add.at(s, row, xyz[idx].astype(np.float64))
        mean = s / r["counts"][:, None]
        R = np.zeros((r["n_voxels"], 3))
        np.maximum.at(R, row, np.abs(xyz[idx].astype(np.float64)))
        R = np.maximum(np.maximum(R, np.abs(np.asarray(o, np.float64))[None, :]), np.abs(r["points"].astype(np.float64)))
        err = np.abs(r["points"].astype(np.float64) - mean)
        bound = v * 2.0 ** -15 + 12 * eps * R
        assert r["n_voxels"] > 300 and (err <= bound).all(), (seed, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    assert worst > 0.05      # (the bound is not vacuous: the error uses a real share of it)


def test_the_generated_clouds_exercise_the_definition():
    """every shape of the issue is in the list; the larger clouds have holes in every coordinate, non-positive disparities,
    voxels with many points and voxels with one, so that min_points and the order matter"""
    shapes = [c[:2] for c in VR.SHAPE_CASES]
    assert shapes == [(1, 1), (1, 63), (1, 64), (3, 257), (48, 320), (97, 331)]
    for i in (4, 5):
        H, W, v, o, mp = VR.SHAPE_CASES[i]
        xyz, disp, col = VR.case_input(i)
        for a in range(3):
            assert (~np.isfinite(xyz[:, :, a])).sum() > 20
        assert (disp <= 0).sum() > 50
        w = VR.case_want(i)
        full = VR.voxel_downsample(xyz.reshape(-1, 3), disp.reshape(-1), None, v, o, 1)
        assert 500 < w["n_voxels"] < H * W // 3 and (full["counts"] == 1).sum() > 10 and full["counts"].max() >= 8
        assert not np.array_equal(np.sort(w["keys"]), w["keys"])          # the order by first is not the order by key
        assert w["n_voxels"] <= full["n_voxels"] and (mp == 1 or w["n_voxels"] < full["n_voxels"])
        assert len(np.unique(w["colors"])) > 100
    assert VR.case_want(0)["n_voxels"] + VR.case_want(1)["n_voxels"] > 10


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; the lists fixed earlier and the ABI version stay"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "sgm_hip_voxel.h")).read()
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", extra, flags=re.S))))
    assert declared == sorted(_lib.VOXEL_EXPORTS) == NEW
    assert '#include "sgm_hip_voxel.h"' in txt and all(hasattr(_lib.load(), n) for n in declared)
    for other in (_lib.EXPORTS, _lib.CONFIDENCE_EXPORTS, _lib.RIGHT_EXPORTS, _lib.WLS_EXPORTS, _lib.WLS_BATCH_EXPORTS, _lib.LRC_EXPORTS):
        assert not set(_lib.VOXEL_EXPORTS) & set(other)
    assert _lib.load().sgm_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define SGM_ABI_VERSION 4\b", txt) and "sgm_hip_voxel.h" in txt.split("typedef enum")[0]
    assert all(callable(getattr(cv.Engine, n)) for n in ("voxel_downsample_host", "voxel_downsample_device"))
    assert callable(cv.voxel_down_sample) and "voxel_down_sample" in cv.__all__
    # the prototypes and the binding agree on the number of arguments
    L = _lib.load()
    for name in NEW:
        proto = re.search(name + r"\s*\((.*?)\);", re.sub(r"/\*.*?\*/", "", extra, flags=re.S), flags=re.S).group(1)
        assert len(proto.split(",")) == len(getattr(L, name).argtypes) == 13
    # what the documents must say: our own definition, not Open3D's
    for doc in (extra, cv.voxel_down_sample.__doc__, open(os.path.join(ROOT, "README.md")).read()):
        assert re.search(r"NOT\s+Open3D", doc.replace("**", ""), flags=re.I)
    # the two debug bits sit above the filter's fields
    dbg = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_debug.h")).read()
    assert re.search(r"SGM_DBG_VOXEL_TIGHT_TABLE = 1 << 22\b", dbg) and re.search(r"SGM_DBG_VOXEL_OTHER_REDUCTION = 1 << 23\b", dbg)
    assert (_lib.SGM_DBG_VOXEL_TIGHT_TABLE, _lib.SGM_DBG_VOXEL_OTHER_REDUCTION) == (1 << 22, 1 << 23)
    assert VR.MAX_POINTS == cv.pointcloud.VOXEL_MAX_POINTS == (1 << 24) - 1 >= 4096 * 2160


def test_the_c_entries_refuse_without_an_engine():
    """a null engine is refused before anything touches the GPU"""
    L = _lib.load()
    org = (np.ctypeslib.ctypes.c_float * 3)(0, 0, 0)
    nv = np.ctypeslib.ctypes.c_int64(-7)
    for fn in (L.sgm_voxel_downsample, L.sgm_voxel_downsample_device):
        assert fn(None, 8, None, None, 4, 0.05, org, 1, 16, None, None, np.ctypeslib.ctypes.byref(nv), None) == -1   # SGM_ERR_INVALID_ARG
        assert b"sgm_voxel_downsample" in L.sgm_last_error() and nv.value == -7


@pytest.fixture()
def no_engine(monkeypatch):
    """any attempt to get an engine fails the test: the errors below are raised in front of it"""
    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(S, "get_engine", boom)
    monkeypatch.setattr(S, "Engine", boom)


def test_voxel_down_sample_argument_errors_come_before_any_engine(no_engine):
    p3, d, c = np.zeros((6, 9, 3), np.float32), np.ones((6, 9), np.float32), np.zeros((6, 9, 3), np.uint8)
    lst = np.zeros((10, 3), np.float32)
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        cv.voxel_down_sample(p3, c, d[:, :8], 0.1)
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        cv.voxel_down_sample(lst, None, d, 0.1)
    with pytest.raises(cv.error, match=r"\(N, 3\) list"):
        cv.voxel_down_sample(p3, c, None, 0.1)
    with pytest.raises(cv.error, match=r"\(N, 3\) list"):
        cv.voxel_down_sample(np.zeros((10, 4), np.float32), None, None, 0.1)
    with pytest.raises(cv.error, match="float32"):
        cv.voxel_down_sample(p3.astype(np.float64), c, d, 0.1)
    with pytest.raises(cv.error, match="colors must be uint8"):
        cv.voxel_down_sample(p3, c[:5], d, 0.1)
    with pytest.raises(cv.error, match="colors must be uint8"):
        cv.voxel_down_sample(p3, c.astype(np.float32), d, 0.1)
    with pytest.raises(cv.error, match="colors must be uint8"):
        cv.voxel_down_sample(lst, np.zeros((9, 3), np.uint8), None, 0.1)
    with pytest.raises(cv.error, match="confidence must have the shape"):
        cv.voxel_down_sample(p3, c, d, 0.1, confidence=np.zeros((6, 8), np.uint8))
    with pytest.raises(cv.error, match="needs a disparity_map"):
        cv.voxel_down_sample(lst, None, None, 0.1, confidence=np.zeros(10, np.uint8))
    for v in (0, -1.0, np.nan, np.inf, 1e-45, 1e39, "x", None, (1, 2)):
        with pytest.raises(cv.error, match="voxel_size"):
            cv.voxel_down_sample(p3, c, d, v)
    for o in ((0, 0), (0, 0, np.nan), (np.inf, 0, 0), 1.0, (0, 0, 0, 0), (1e39, 0, 0)):
        with pytest.raises(cv.error, match="origin"):
            cv.voxel_down_sample(p3, c, d, 0.1, origin=o)
    for mp in (0, -3, 1.5, True, None, "2", 2 ** 31):
        with pytest.raises(cv.error, match="min_points"):
            cv.voxel_down_sample(p3, c, d, 0.1, min_points=mp)
    import inspect
    assert list(inspect.signature(cv.voxel_down_sample).parameters) == [
        "points_3D", "colors", "disparity_map", "voxel_size", "origin", "min_points", "confidence", "min_confidence", "return_counts"]
