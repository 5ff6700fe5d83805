"""Statistical outlier removal without a GPU: hand-worked answers of the definition (include/sgm_hip_statistical.h) held against
its numpy restatement tests/statistical_ref.py, the two forms of the reference against each other, the kept-share table, the
invariance under the order of the points, the bound on q measured, the interface lists (header, binding, library, ABI version)
and the Python argument errors, all of which are raised before any engine exists.  What the device computes is held against
statistical_ref.py in tests/test_gpu_statistical.py."""
import inspect
import os
import re

import numpy as np
import pytest

import statistical_ref as SR
import stereo_reconstruction_cv_amd as cv
from stereo_reconstruction_cv_amd import _lib
from stereo_reconstruction_cv_amd import stereo as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sgm_statistical_outlier", "sgm_statistical_outlier_device"]
F32 = np.float32


def f32(x):
    return np.asarray(x, np.float32)


def same(a, b):
    for k in ("keep", "index", "q", "dense", "in_range", "stats"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["mean"].view(np.uint32), b["mean"].view(np.uint32))
    assert np.array_equal(a["points"].view(np.uint32), b["points"].view(np.uint32))
    assert (a["colors"] is None) == (b["colors"] is None) and (a["colors"] is None or np.array_equal(a["colors"], b["colors"]))
    assert a["n_kept"] == b["n_kept"]


def both(xyz, disp=None, colors=None, **kw):
    a, b = SR.brute(f32(xyz), disp, colors, **kw), SR.cells(f32(xyz), disp, colors, **kw)
    same(a, b)
    return a


def stats(r):
    return dict(zip(SR.STATS, (int(x) for x in r["stats"])))


# ---- the definition, by hand -----------------------------------------------------------------------------------------------------
def test_three_collinear_points_with_k_1():
    """x = 0, 0.25, 0.75 and r = 1: qscale = 2^19 and every step is exact.  The nearest neighbours are 0.25, 0.25 and 0.5 away:
    q = 2^17, 2^17, 2^18; A = 2^19; B = 2^34 + 2^34 + 2^36.  mu = 174762.67, the deviations are -43690.67 twice and 87381.33, so
    var = 11453246122.67 / 2 and its root is 75674.45: thr = 250437.1 at std_ratio 1 keeps the first two, 326111.6 at 2 all."""
    pts = [[0, 0, 0], [0.25, 0, 0], [0.75, 0, 0]]
    r = both(pts, nb_neighbors=1, std_ratio=1.0, max_radius=1.0)
    assert r["mean"].tolist() == [0.25, 0.25, 0.5] and r["q"].tolist() == [1 << 17, 1 << 17, 1 << 18]
    assert stats(r) == dict(in_range=3, out_of_range=0, dense=3, sparse=0, A=1 << 19, B=(1 << 35) + (1 << 36), T=250437)
    assert r["keep"].tolist() == [1, 1, 0] and r["index"].tolist() == [0, 1] and r["n_kept"] == 2
    r = both(pts, nb_neighbors=1, std_ratio=2.0, max_radius=1.0)
    assert stats(r)["T"] == 326111 and r["keep"].tolist() == [1, 1, 1]


def test_three_collinear_points_with_k_2_and_the_inclusive_threshold():
    """the same points, k = 2: the means are (0.25 + 0.75) / 2, (0.25 + 0.5) / 2, (0.5 + 0.75) / 2, q = 4, 3 and 5 times 2^16;
    mu = 2^18, var = (2^32 + 2^32) / 2, so thr = 2^18 + 2^16 exactly at std_ratio 1: the third point has q == T and is kept"""
    pts = [[0, 0, 0], [0.25, 0, 0], [0.75, 0, 0]]
    r = both(pts, nb_neighbors=2, std_ratio=1.0, max_radius=1.0)
    assert r["mean"].tolist() == [0.5, 0.375, 0.625] and r["q"].tolist() == [4 << 16, 3 << 16, 5 << 16]
    s = stats(r)
    assert (s["A"], s["B"], s["T"]) == (12 << 16, 50 << 32, 5 << 16) and r["keep"].tolist() == [1, 1, 1]
    # std_ratio 0: T = floor(mu), and the point at the mean itself is kept
    r = both(pts, nb_neighbors=2, std_ratio=0.0, max_radius=1.0)
    assert stats(r)["T"] == 1 << 18 and r["keep"].tolist() == [1, 1, 0]
    # a std_ratio just under 1 (0.99999994) puts thr under 5 * 2^16: the third point goes
    r = both(pts, nb_neighbors=2, std_ratio=np.nextafter(F32(1), F32(0)), max_radius=1.0)
    assert stats(r)["T"] == (5 << 16) - 1 and r["keep"].tolist() == [1, 1, 0]


def test_exactly_k_and_k_minus_1_neighbours_and_a_single_dense_point():
    """x = 0, 0.25, 0.5 with r = 0.25: the middle point has two neighbours at exactly r (the test is inclusive), the ends one.
    k = 2: the middle is the only dense point, m = 1, var = 0, T = its q = 0.25 * (2^19 / 0.25) = 2^19"""
    pts = [[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0]]
    r = both(pts, nb_neighbors=2, std_ratio=1.0, max_radius=0.25)
    assert r["dense"].tolist() == [False, True, False] and r["mean"].tolist() == [-1.0, 0.25, -1.0]
    assert stats(r) == dict(in_range=3, out_of_range=0, dense=1, sparse=2, A=1 << 19, B=1 << 38, T=1 << 19)
    assert r["keep"].tolist() == [0, 1, 0]
    r = both(pts, nb_neighbors=1, std_ratio=1.0, max_radius=0.25)
    assert r["dense"].all() and r["q"].tolist() == [1 << 19] * 3 and r["n_kept"] == 3 and stats(r)["T"] == 1 << 19
    r = both(pts, nb_neighbors=3, std_ratio=1.0, max_radius=0.25)       # m = 0: nothing kept, T = 0
    assert stats(r) == dict(in_range=3, out_of_range=0, dense=0, sparse=3, A=0, B=0, T=0) and r["n_kept"] == 0
    assert r["mean"].tolist() == [-1.0] * 3 and r["points"].shape == (0, 3)


def test_duplicates_have_mean_0_and_a_point_does_not_count_itself():
    pts = [[1, 2, 3]] * 5 + [[9, 9, 9]]
    col = np.arange(18, dtype=np.uint8).reshape(6, 3)
    r = both(pts, colors=col, nb_neighbors=4, std_ratio=1.0, max_radius=0.125)
    assert r["mean"].tolist() == [0.0] * 5 + [-1.0] and r["q"].tolist() == [0] * 6 and r["keep"].tolist() == [1] * 5 + [0]
    assert stats(r) == dict(in_range=6, out_of_range=0, dense=5, sparse=1, A=0, B=0, T=0)
    assert r["colors"].tolist() == col[:5].tolist() and r["index"].tolist() == [0, 1, 2, 3, 4]
    # five copies have four neighbours each, not five
    r = both(pts, nb_neighbors=5, std_ratio=1.0, max_radius=0.125)
    assert not r["dense"].any() and r["n_kept"] == 0 and stats(r)["sparse"] == 6
    assert both([[1, 2, 3]], nb_neighbors=1, std_ratio=1.0, max_radius=0.125)["dense"].tolist() == [False]


def test_validity_and_range_are_the_radius_filter_s():
    pts = f32([[0, 0, 0], [0.25, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0.25, 0], [3e38, 0, 0]])
    disp = f32([1, 1, 1, 1, 0, 1])
    r = both(pts, disp, nb_neighbors=1, std_ratio=1.0, max_radius=0.5)
    assert r["in_range"].tolist() == [True, True, False, False, False, False] and r["mean"].tolist() == [0.25, 0.25, -1, -1, -1, -1]
    assert stats(r)["out_of_range"] == 1 and r["keep"].tolist() == [1, 1, 0, 0, 0, 0]
    r = both(pts, None, nb_neighbors=2, std_ratio=1.0, max_radius=0.5)
    assert r["dense"].tolist() == [True, True, False, False, True, False]
    want = F32(F32(0.25) + np.sqrt(F32(0.125))) / F32(2)
    assert r["mean"][[0, 1, 4]].tolist() == [0.25, float(want), float(want)]


def test_the_k_smallest_are_summed_in_ascending_order():
    """one centre with neighbours at distances whose float32 sum depends on the order: the definition adds them ascending"""
    rng = np.random.default_rng(8)
    d = np.sort(rng.random(12).astype(np.float32) * F32(0.4) + F32(1e-3))
    pts = np.zeros((13, 3), np.float32)
    pts[1:, 0] = d * np.where(np.arange(12) % 2, F32(-1), F32(1))       # both sides of the centre, far from each other or not
    r = both(pts, nb_neighbors=7, std_ratio=1.0, max_radius=0.5)
    s = np.sqrt(np.sort(d * d))[:7]
    acc = s[0]
    for x in s[1:]:
        acc = F32(acc + x)
    assert r["dense"][0] and r["mean"][0] == F32(acc / F32(7))


# ---- the two forms, the table, the properties ----------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SR.SHAPE_CASES)))
def test_the_two_forms_agree_on_the_case_table(i):
    kind, a, b, k, ratio, r, o = SR.SHAPE_CASES[i]
    xyz, disp, col = SR.case_input(i)
    same(SR.brute(xyz, disp, col, k, ratio, r, o), SR.case_want(i))
    if kind == "layered" and a == 24:
        same(SR.brute(xyz, None, col, k, ratio, r, o), SR.case_want(i, with_disp=False))


def test_the_case_table_has_every_shape_and_dense_and_sparse_points():
    shapes = [c[1] if c[0] == "list" else c[1:3] for c in SR.SHAPE_CASES]
    assert shapes[:6] == [1, 2, 63, 64, 65, 257] and (24, 130) in shapes and (48, 320) in shapes
    for i in range(2, len(SR.SHAPE_CASES)):
        s = stats(SR.case_want(i))
        assert s["dense"] > 0 and s["sparse"] > 0 and 0 < SR.case_want(i)["n_kept"] < s["dense"], (i, s)


@pytest.mark.parametrize("row", SR.SHARE_ROWS)
def test_the_kept_share_rows(row):
    H, W, seed, r, k, ratio, dense, sparse, kept, T = row
    w = SR.layered_want(H, W, seed, k, ratio, r)
    s = stats(w)
    assert (s["dense"], s["sparse"], w["n_kept"], s["T"]) == (dense, sparse, kept, T)
    assert s["in_range"] == (13576 if H == 48 else 2745) and 0.05 < w["n_kept"] / s["in_range"] < 0.95


def test_the_sparse_dominated_row():
    H, W, seed, r, k, ratio, dense, sparse, kept = SR.SPARSE_ROW
    w = SR.layered_want(H, W, seed, k, ratio, r)
    assert (stats(w)["dense"], stats(w)["sparse"], w["n_kept"]) == (dense, sparse, kept)


def test_nothing_depends_on_the_order_of_the_points():
    xyz, disp, col = SR.layered_lists(24, 130, 724)
    a = SR.layered_want(24, 130, 724, 4, 1.0, 0.03)
    b = SR.cells(xyz[::-1].copy(), disp[::-1].copy(), col[::-1].copy(), 4, 1.0, 0.03)
    assert np.array_equal(a["mean"].view(np.uint32), b["mean"][::-1].view(np.uint32)) and np.array_equal(a["keep"], b["keep"][::-1])
    assert np.array_equal(a["stats"], b["stats"]) and np.array_equal(a["points"].view(np.uint32), b["points"][::-1].view(np.uint32))


def test_the_bound_on_q_measured():
    """q < 2^19 + 4.  The largest q belongs to a point all of whose k nearest are at exactly r2: one point with k others r away
    along an axis (d2 = r * r = r2), at random radii, with one addition and with 63"""
    worst = max(int(SR.case_want(i)["q"].max()) for i in range(len(SR.SHAPE_CASES)))
    assert worst < 1 << 19
    rng = np.random.default_rng(12)
    top = 0
    for r in np.exp(rng.uniform(np.log(1e-3), np.log(50.0), size=300)).astype(np.float32):
        for k in (1, 64):
            pts = np.zeros((k + 1, 3), np.float32)
            pts[1:, 0] = r
            res = SR.brute(pts, None, None, k, 1.0, r)
            assert res["dense"][0]
            top = max(top, int(res["q"].max()))
    assert (1 << 19) <= top < (1 << 19) + 4, top


def test_step_8_in_binary64():
    assert SR.threshold(0, 0, 0, 1.0) == 0 and SR.threshold(1, 77, 77 * 77, 3.0) == 77
    assert SR.threshold(2, 10, 52, 1.0) == 5 + 1         # q = 4, 6: mu 5, var 2, floor(6.414)
    assert SR.threshold(2, 10, 52, 0.0) == 5
    assert SR.threshold(3, 3 << 19, 3 << 38, 1.0) == 1 << 19          # equal values: var is exactly 0
    assert SR.threshold(2, 10, 52, 3e38) == 2 ** 32 - 2               # clamped: every dense point is kept


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; the lists fixed earlier and the ABI version stay"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "sgm_hip_statistical.h")).read()
    code = re.sub(r"/\*.*?\*/", "", extra, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", code)))
    L = _lib.load()
    assert declared == sorted(_lib.STATISTICAL_EXPORTS) == NEW
    assert '#include "sgm_hip_statistical.h"' in txt and all(hasattr(L, n) for n in declared)
    assert txt.index('#include "sgm_hip_radius.h"') < txt.index('#include "sgm_hip_statistical.h"')
    earlier = dict(EXPORTS=34, CONFIDENCE_EXPORTS=1, RIGHT_EXPORTS=1, WLS_EXPORTS=3, WLS_BATCH_EXPORTS=2, LRC_EXPORTS=3,
                   VOXEL_EXPORTS=2, MESH_EXPORTS=2, NORMALS_EXPORTS=4, RADIUS_EXPORTS=2)
    for name, length in earlier.items():
        other = getattr(_lib, name)
        assert not set(_lib.STATISTICAL_EXPORTS) & set(other) and (length is None or len(other) == length), name
    assert _lib.RADIUS_EXPORTS == ("sgm_radius_outlier", "sgm_radius_outlier_device")
    assert L.sgm_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define SGM_ABI_VERSION 4\b", txt) and "sgm_hip_statistical.h" in txt.split("typedef enum")[0]
    assert all(callable(getattr(cv.Engine, n)) for n in ("statistical_outlier_host", "statistical_outlier_device"))
    assert callable(cv.remove_statistical_outlier) and "remove_statistical_outlier" in cv.__all__
    for name in NEW:      # the prototypes and the binding agree on the number of arguments
        proto = re.search(name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(getattr(L, name).argtypes) == 16
    readme = open(os.path.join(ROOT, "README.md")).read()
    for doc in (extra, cv.remove_statistical_outlier.__doc__, readme):
        assert re.search(r"NOT\s+Open3D", doc.replace("**", ""), flags=re.I)
    for doc in (extra, cv.remove_statistical_outlier.__doc__):
        assert re.search(r"a\s+few\s+times", doc)
    radius_h = open(os.path.join(ROOT, "include", "sgm_hip_radius.h")).read()
    assert "sgm_hip_statistical.h" in radius_h and "are not offered" not in radius_h
    assert SR.MAX_K == cv.pointcloud.STATISTICAL_MAX_NEIGHBORS == 64
    dbg = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_debug.h")).read()
    assert re.search(r"SGM_DBG_STAT_WIDE_LIST = 1 << 26\b", dbg) and _lib.SGM_DBG_STAT_WIDE_LIST == 1 << 26
    assert list(inspect.signature(cv.remove_statistical_outlier).parameters) == [
        "points_3D", "colors", "disparity_map", "nb_neighbors", "std_ratio", "max_radius", "origin", "confidence", "min_confidence",
        "return_mask", "return_distances", "return_index", "return_stats"]


def test_the_c_entries_refuse_without_an_engine():
    """a null engine is refused before anything touches the GPU"""
    import ctypes as C
    L = _lib.load()
    org = (C.c_float * 3)(0, 0, 0)
    nk = C.c_int64(-7)
    for fn in (L.sgm_statistical_outlier, L.sgm_statistical_outlier_device):
        assert fn(None, 8, None, None, 4, 2, 1.0, 0.05, org, None, None, 16, None, None, C.byref(nk), None) == -1   # SGM_ERR_INVALID_ARG
        assert b"sgm_statistical_outlier" in L.sgm_last_error() and nk.value == -7


@pytest.fixture()
def no_engine(monkeypatch):
    """any attempt to get an engine fails the test: the errors below are raised in front of it"""
    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(S, "get_engine", boom)
    monkeypatch.setattr(S, "Engine", boom)


def test_remove_statistical_outlier_argument_errors_come_before_any_engine(no_engine):
    p3, d, c = np.zeros((6, 9, 3), np.float32), np.ones((6, 9), np.float32), np.zeros((6, 9, 3), np.uint8)
    lst = np.zeros((10, 3), np.float32)
    rso = cv.remove_statistical_outlier
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        rso(p3, c, d[:, :8], 4, 1.0, 0.1)
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        rso(lst, None, d, 4, 1.0, 0.1)
    with pytest.raises(cv.error, match=r"\(N, 3\) list"):
        rso(p3, c, None, 4, 1.0, 0.1)
    with pytest.raises(cv.error, match=r"\(N, 3\) list"):
        rso(np.zeros((10, 4), np.float32), None, None, 4, 1.0, 0.1)
    with pytest.raises(cv.error, match="remove_statistical_outlier: points_3D must be float32"):
        rso(p3.astype(np.float64), c, d, 4, 1.0, 0.1)
    for bad in (c[:5], c.astype(np.float32)):
        with pytest.raises(cv.error, match="colors must be uint8"):
            rso(p3, bad, d, 4, 1.0, 0.1)
    with pytest.raises(cv.error, match="confidence must have the shape"):
        rso(p3, c, d, 4, 1.0, 0.1, confidence=np.zeros((6, 8), np.uint8))
    with pytest.raises(cv.error, match="needs a disparity_map"):
        rso(lst, None, None, 4, 1.0, 0.1, confidence=np.zeros(10, np.uint8))
    for k in (0, -3, 65, 1.5, True, None, "2", 2 ** 31):
        with pytest.raises(cv.error, match="nb_neighbors"):
            rso(p3, c, d, k, 1.0, 0.1)
    for ratio in (-1.0, -1e-30, np.nan, np.inf, 1e39, "x", None, (1, 2), True):
        with pytest.raises(cv.error, match="std_ratio"):
            rso(p3, c, d, 4, ratio, 0.1)
    for r in (0, -1.0, np.nan, np.inf, 1e-45, 1e-20, 1e20, 1e39, "x", None, (1, 2)):     # 1e-20, 1e20: the square leaves the normal range
        with pytest.raises(cv.error, match="max_radius"):
            rso(p3, c, d, 4, 1.0, r)
    for o in ((0, 0), (0, 0, np.nan), (np.inf, 0, 0), 1.0, (0, 0, 0, 0), (1e39, 0, 0)):
        with pytest.raises(cv.error, match="origin"):
            rso(p3, c, d, 4, 1.0, 0.1, origin=o)
    # an empty list needs no engine either
    out = rso(np.zeros((0, 3), np.float32), None, None, 4, 1.0, 0.1, return_mask=True, return_distances=True, return_index=True, return_stats=True)
    assert out[0].shape == (0, 3) and out[1] is None and [a.shape for a in out[2:5]] == [(0,)] * 3
    assert out[5] == dict(in_range=0, out_of_range=0, dense=0, sparse=0, A=0, B=0, T=0)
    # the radius function's errors are what they were
    with pytest.raises(cv.error, match="remove_radius_outlier: points_3D must be float32"):
        cv.remove_radius_outlier(p3.astype(np.float64), c, d, 4, 0.1)
