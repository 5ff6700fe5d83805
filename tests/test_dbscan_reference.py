"""Density clustering without a GPU: hand-worked answers of the definition (include/sgm_hip_dbscan.h) held against its numpy
restatement tests/dbscan_ref.py, the border rule and its tie, the numbering, the core mask against the radius filter's keep mask,
the two forms of the reference against each other, the invariances under the order of the points and under a power-of-two scale,
long chains, largest_clusters, the interface lists (header, binding, library, stage names, debug bit), the Python argument errors,
all of which are raised before any engine exists, the scratch memory of the kernels, and the condition on the generated clouds that
keeps the GPU tests from passing on a cloud that is all noise or all one cluster.  What the device computes is held against
dbscan_ref.py in tests/test_gpu_dbscan.py."""
import inspect
import os
import re

import numpy as np
import pytest

import dbscan_ref as DR
import radius_ref as RR
import stereo_reconstruction_cv_amd as cv
from stereo_reconstruction_cv_amd import _lib
from stereo_reconstruction_cv_amd import stereo as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sgm_cluster_dbscan", "sgm_cluster_dbscan_device"]
F32 = np.float32
NCASE = len(DR.SHAPE_CASES)
KEYS = ("labels", "core", "sizes", "stats", "in_range")


def f32(x):
    return np.asarray(x, np.float32)


def same(a, b):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert a["n_clusters"] == b["n_clusters"] == a["sizes"].size == int(a["stats"][5])


def both(xyz, disp=None, **kw):
    a, b = DR.brute(f32(xyz), disp, **kw), DR.cells(f32(xyz), disp, **kw)
    same(a, b)
    assert a["labels"].dtype == np.int32 and a["core"].dtype == np.uint8 and a["sizes"].dtype == np.uint32 and a["stats"].dtype == np.uint64
    return a


def stats(r):
    return dict(zip(DR.STATS, (int(x) for x in r["stats"])))


# ---- the definition, by hand -----------------------------------------------------------------------------------------------------
def test_three_collinear_points():
    """0, 0.5, 1 on the x axis, eps 0.6: the ends have one neighbour, the middle two.  k = 1: all core, one cluster.  k = 2: the
    middle alone is core and the ends are its border points.  k = 3: nothing is core and everything noise."""
    pts = [[0, 0, 0], [0.5, 0, 0], [1, 0, 0]]
    r = both(pts, eps=0.6, min_points=1)
    assert r["labels"].tolist() == [0, 0, 0] and r["core"].tolist() == [1, 1, 1] and r["sizes"].tolist() == [3]
    assert stats(r) == dict(in_range=3, out_of_range=0, core=3, border=0, noise=0, clusters=1)
    r = both(pts, eps=0.6, min_points=2)
    assert r["labels"].tolist() == [0, 0, 0] and r["core"].tolist() == [0, 1, 0] and r["sizes"].tolist() == [3]
    assert stats(r) == dict(in_range=3, out_of_range=0, core=1, border=2, noise=0, clusters=1)
    r = both(pts, eps=0.6, min_points=3)
    assert r["labels"].tolist() == [-1, -1, -1] and r["core"].tolist() == [0, 0, 0] and r["sizes"].size == 0
    assert stats(r) == dict(in_range=3, out_of_range=0, core=0, border=0, noise=3, clusters=0)


def test_two_points_at_exactly_eps_and_one_ulp_beyond():
    r = both([[0, 0, 0], [0.25, 0, 0]], eps=0.25, min_points=1)            # d2 == r2 exactly: the test is inclusive
    assert r["labels"].tolist() == [0, 0] and r["sizes"].tolist() == [2]
    q = DR.beyond([0, 0, 0], (1, 0, 0), 0.25)
    assert q[0] == np.nextafter(F32(0.25), F32(1))
    r = both([[0, 0, 0], q], eps=0.25, min_points=1)
    assert r["labels"].tolist() == [-1, -1] and stats(r)["noise"] == 2


def test_duplicates_only():
    """five copies of one point: each has four neighbours at d2 = 0"""
    pts = np.tile(f32([[0.3, -0.2, 1.7]]), (5, 1))
    r = both(pts, eps=0.05, min_points=4)
    assert r["labels"].tolist() == [0] * 5 and r["core"].tolist() == [1] * 5 and r["sizes"].tolist() == [5]
    r = both(pts, eps=0.05, min_points=5)
    assert r["labels"].tolist() == [-1] * 5 and stats(r)["noise"] == 5


def test_an_isolated_point_invalid_points_and_points_out_of_range_are_noise():
    pts = f32([[0, 0, 0], [0.1, 0, 0], [5, 5, 5], [np.nan, 0, 0], [3e7, 0, 0], [0.05, 0.05, 0]])
    disp = f32([1, 1, 1, 1, 1, 0])
    r = both(pts, disp, eps=0.2, min_points=1)
    assert r["labels"].tolist() == [0, 0, -1, -1, -1, -1] and r["core"].tolist() == [1, 1, 0, 0, 0, 0]
    assert stats(r) == dict(in_range=3, out_of_range=1, core=2, border=0, noise=1, clusters=1)


# ---- the border rule ---------------------------------------------------------------------------------------------------------------
def clump(tip, sign):
    """four points that are one another's neighbours at eps = 0.25, of which only the first -- the tip, on the x axis at `tip` -- is
    within eps of the origin: the other three sit 0.125 farther along sign.  Every coordinate is a dyadic fraction: all d2 are exact."""
    x = tip + sign * 0.125
    return [[tip, 0, 0], [x, 0.0625, 0], [x, -0.0625, 0], [x, 0, 0.0625]]


def test_a_border_point_between_two_clusters_does_not_merge_them_and_goes_to_the_nearer():
    """the origin between the tips of two clumps has two neighbours, both core at k = 3: it is a border point, joins the nearer
    tip's cluster and leaves the two clusters apart; at k = 2 it is core itself and the three are one cluster"""
    for tl, tr, want in ((-0.1875, 0.125, 1), (-0.125, 0.1875, 0), (-0.25, 0.1875, 1), (-0.125, 0.25, 0)):
        pts = clump(tl, -1) + clump(tr, 1) + [[0, 0, 0]]
        r = both(pts, eps=0.25, min_points=3)
        assert r["core"].tolist() == [1] * 8 + [0] and r["n_clusters"] == 2, (tl, tr)
        assert r["labels"].tolist() == [0] * 4 + [1] * 4 + [want] and r["sizes"].tolist() == [4 + (want == 0), 4 + (want == 1)]
        assert stats(r) == dict(in_range=9, out_of_range=0, core=8, border=1, noise=0, clusters=2)
        r = both(pts, eps=0.25, min_points=2)
        assert r["core"].tolist() == [1] * 9 and r["labels"].tolist() == [0] * 9 and r["sizes"].tolist() == [9]


def test_an_equidistant_border_point_goes_to_the_lower_source_index():
    """the origin at exactly 0.1875 of both tips: the same d2 bits, so the lower index decides -- and with the clumps swapped in the
    list the other clump has it"""
    left, right, mid = clump(-0.1875, -1), clump(0.1875, 1), [[0, 0, 0]]
    d = RR.d2_of(f32(mid[0]), f32([left[0], right[0]]))
    assert d[0].view(np.uint32) == d[1].view(np.uint32)
    r = both(left + right + mid, eps=0.25, min_points=3)
    assert r["core"].tolist() == [1] * 8 + [0] and r["labels"].tolist() == [0] * 4 + [1] * 4 + [0]
    r = both(right + left + mid, eps=0.25, min_points=3)
    assert r["labels"].tolist() == [0] * 4 + [1] * 4 + [0] and r["sizes"].tolist() == [5, 4]      # cluster 0 is the right clump now
    r = both(mid + right + left, eps=0.25, min_points=3)
    assert r["labels"].tolist() == [0] + [0] * 4 + [1] * 4
    # the nearest CORE point: at k = 4 the tips alone are core (five neighbours), and a point beside the origin, nearer to it than
    # either tip, is no core point and changes nothing
    r = both(left + right + mid + [[0, 0.0078125, 0]], eps=0.25, min_points=4)
    assert r["core"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 0, 0] and r["labels"].tolist() == [0] * 4 + [1] * 4 + [0, 0]
    assert stats(r) == dict(in_range=10, out_of_range=0, core=2, border=8, noise=0, clusters=2)


def test_numbering_by_the_smallest_core_index():
    """two clumps, the second clump's points first in the list except that a border point of the first clump has index 0: cluster 0
    is the clump whose smallest CORE index is the smaller, whatever its border points' indices"""
    a = [[0.05 * i, 0.05 * (i % 2), 0] for i in range(4)]                    # four points, all core at k = 3
    b = [[5 + 0.05 * i, 0.05 * (i % 2), 0] for i in range(4)]
    border_of_b = [[5 + 0.15 + 0.24, 0.05, 0]]                               # within eps of b's last point only
    r = both(border_of_b + a + b, eps=0.25, min_points=3)
    assert r["core"].tolist() == [0] + [1] * 8
    assert r["labels"].tolist() == [1] + [0] * 4 + [1] * 4 and r["sizes"].tolist() == [4, 5]
    assert r["representatives"].tolist() == [1, 5]
    r = both(border_of_b + b + a, eps=0.25, min_points=3)
    assert r["labels"].tolist() == [0] + [0] * 4 + [1] * 4 and r["sizes"].tolist() == [5, 4] and r["representatives"].tolist() == [1, 5]


# ---- the case table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NCASE))
def test_the_core_mask_is_the_keep_mask_of_the_radius_filter(i):
    eps, k, o = DR.SHAPE_CASES[i][3:]
    xyz, disp = DR.case_input(i)
    keep = RR.cells(xyz, disp, None, eps, k, k, o)
    want = DR.case_want(i)
    assert want["core"].tobytes() == keep["keep"].tobytes() and int(want["stats"][1]) == keep["n_out_of_range"]
    assert np.array_equal(want["in_range"], keep["in_range"])


@pytest.mark.parametrize("i", range(NCASE))
def test_the_two_forms_agree_on_the_case_table(i):
    eps, k, o = DR.SHAPE_CASES[i][3:]
    xyz, disp = DR.case_input(i)
    if xyz.shape[0] > 5000:                   # the dense form on the first 5000 points of the larger clouds
        xyz, disp = xyz[:5000], disp[:5000]
        same(DR.brute(xyz, disp, eps, k, o), DR.cells(xyz, disp, eps, k, o))
    else:
        same(DR.brute(xyz, disp, eps, k, o), DR.case_want(i))
        if disp is not None:
            same(DR.brute(xyz, None, eps, k, o), DR.case_want(i, False))
    w = DR.case_want(i)
    s = stats(w)
    assert s["core"] + s["border"] + s["noise"] == s["in_range"] and int(w["sizes"].sum()) == s["core"] + s["border"]
    assert (w["labels"][w["core"] > 0] >= 0).all() and (w["labels"][~w["in_range"]] == -1).all()
    assert sorted(set(w["labels"].tolist()) - {-1}) == list(range(s["clusters"]))


def test_the_generated_clouds_have_clusters_core_border_and_noise():
    """a condition, not a measurement: at least three layered rows of the case table in which the reference alone finds at least 3
    clusters and core, border and noise points are each at least 5 % of the points in range"""
    good = 0
    for i in DR.LAYERED_ROWS:
        s = stats(DR.case_want(i))
        assert s["in_range"] > 2000
        good += s["clusters"] >= 3 and min(s["core"], s["border"], s["noise"]) >= 0.05 * s["in_range"]
    assert good >= 3, good
    assert all(DR.case_input(i)[0].shape[0] > 10000 for i in DR.LAYERED_ROWS[1:])


# ---- invariance ----------------------------------------------------------------------------------------------------------------------
def _moved(res, perm):
    """res of the points xyz[perm] brought back to the order of xyz: the partition and the core mask"""
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    parts = sorted(tuple(sorted(perm[list(c)].tolist())) for c in DR.partition(res))
    return parts, res["core"][inv]


@pytest.mark.parametrize("i", [5, 6, 7, 9])
def test_reversal_and_a_permutation_renumber_the_labels_only(i):
    eps, k, o = DR.SHAPE_CASES[i][3:]
    xyz, disp = DR.case_input(i)
    w = DR.case_want(i)
    n = xyz.shape[0]
    for perm in (np.arange(n)[::-1].copy(), np.random.default_rng(11).permutation(n)):
        r = DR.cells(xyz[perm], None if disp is None else disp[perm], eps, k, o)
        parts, core = _moved(r, perm)
        assert parts == DR.partition(w) and np.array_equal(core, w["core"])
        assert r["stats"].tolist() == w["stats"].tolist() and sorted(r["sizes"].tolist()) == sorted(w["sizes"].tolist())


@pytest.mark.parametrize("e", [10, -10, 40, -40])
def test_scaling_by_a_power_of_two_changes_nothing(e):
    s = F32(2.0) ** e
    for i in (6, 7):
        eps, k, o = DR.SHAPE_CASES[i][3:]
        xyz, disp = DR.case_input(i)
        r = DR.cells(xyz * s, disp, F32(eps) * s, k, tuple(f32(o) * s))
        same(r, DR.case_want(i))


# ---- chains ----------------------------------------------------------------------------------------------------------------------------
def test_a_chain_of_3000_points_is_one_cluster_and_two_an_ulp_apart_are_two():
    a, b = DR.two_chains(3000, 0.1)
    r = both(a, eps=0.1, min_points=1)
    assert r["labels"].tolist() == [0] * 3000 and r["sizes"].tolist() == [3000] and stats(r)["core"] == 3000
    r = both(a, eps=0.1, min_points=2)                                       # the two ends are border points
    assert r["core"].tolist() == [0] + [1] * 2998 + [0] and r["sizes"].tolist() == [3000]
    r2 = RR.constants(0.1)[0]
    d = RR.d2_of(a[:8, None, :], b[None, :8, :])
    assert d.min() == d[0, 0] == np.nextafter(r2, F32(1)) or (d.min() == d[0, 0] > r2 and DR.beyond(a[0], (-1, 0, 0), 0.1)[0] == b[0, 0])
    two = np.concatenate([a, b])
    r = DR.cells(two, None, 0.1, 1)
    assert r["labels"].tolist() == [0] * 3000 + [1] * 3000 and r["sizes"].tolist() == [3000, 3000]
    nearer = np.array(two)
    nearer[3000, 0] = np.nextafter(nearer[3000, 0], F32(1))                  # one ulp nearer: one cluster
    r = DR.cells(nearer, None, 0.1, 1)
    assert r["labels"].tolist() == [0] * 6000 and r["sizes"].tolist() == [6000]
    perm = np.random.default_rng(5).permutation(6000)                        # and with the indices shuffled along the chains
    r = DR.cells(two[perm], None, 0.1, 1)
    assert r["n_clusters"] == 2 and _moved(r, perm)[0] == [tuple(range(3000)), tuple(range(3000, 6000))]


def test_the_stripes_of_a_lattice_in_closed_form():
    p, keep = DR.stripes(20, 30, 0.25, 8)
    r = both(p, eps=0.26, min_points=2)
    assert r["sizes"].tolist() == [210, 210, 120] and r["core"].all()
    assert r["labels"].tolist() == [0] * 210 + [1] * 210 + [2] * 120


# ---- largest_clusters --------------------------------------------------------------------------------------------------------------------
def test_largest_clusters():
    labels = np.array([[0, 1, 1, -1], [2, 2, 3, 3], [4, 4, 4, -1]], np.int32)
    sizes = np.array([1, 2, 2, 2, 3], np.uint32)
    lc = cv.largest_clusters
    m = lc(labels, sizes)
    assert m.dtype == np.uint8 and m.shape == labels.shape and m.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 0]]
    assert lc(labels, sizes, count=2).tolist() == [[0, 1, 1, 0], [0, 0, 0, 0], [1, 1, 1, 0]]      # the tie of 1, 2, 3: the lower label
    assert lc(labels, sizes, count=3).tolist() == [[0, 1, 1, 0], [1, 1, 0, 0], [1, 1, 1, 0]]
    assert lc(labels, sizes, count=9).tolist() == [[1, 1, 1, 0], [1, 1, 1, 1], [1, 1, 1, 0]]
    assert lc(labels, sizes, count=9, min_size=2).tolist() == [[0, 1, 1, 0], [1, 1, 1, 1], [1, 1, 1, 0]]
    assert lc(labels, sizes, count=2, min_size=3).tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 0]]
    assert lc(labels, sizes, count=1, min_size=4).sum() == 0 and lc(labels, sizes, count=0).sum() == 0
    assert lc(np.full(5, -1, np.int32), np.zeros(0, np.uint32)).tolist() == [0] * 5
    assert lc(np.zeros(0, np.int32), np.zeros(0, np.uint32)).shape == (0,)
    for bad in (dict(count=-1), dict(count=1.5), dict(count=True), dict(min_size=0), dict(min_size=None)):
        with pytest.raises(cv.error, match="largest_clusters"):
            lc(labels, sizes, **bad)
    with pytest.raises(cv.error, match="int32"):
        lc(labels.astype(np.int64), sizes)
    with pytest.raises(cv.error, match="not below"):
        lc(labels, sizes[:4])
    # on a reference result
    w = DR.case_want(8)
    m = lc(w["labels"], w["sizes"])
    top = int(np.argmax(w["sizes"]))
    assert int(m.sum()) == int(w["sizes"].max()) and np.array_equal(m > 0, w["labels"] == top)


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; the lists fixed earlier and the ABI version stay"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "sgm_hip_dbscan.h")).read()
    code = re.sub(r"/\*.*?\*/", "", extra, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", code)))
    L = _lib.load()
    assert declared == sorted(_lib.DBSCAN_EXPORTS) == NEW
    assert '#include "sgm_hip_dbscan.h"' in txt and all(hasattr(L, n) for n in declared)
    assert txt.index('#include "sgm_hip_covariance.h"') < txt.index('#include "sgm_hip_dbscan.h"')
    earlier = dict(EXPORTS=34, CONFIDENCE_EXPORTS=1, RIGHT_EXPORTS=1, WLS_EXPORTS=3, WLS_BATCH_EXPORTS=2, LRC_EXPORTS=3,
                   VOXEL_EXPORTS=2, MESH_EXPORTS=2, NORMALS_EXPORTS=4, RADIUS_EXPORTS=2, STATISTICAL_EXPORTS=2, COVARIANCE_EXPORTS=2)
    for name, length in earlier.items():
        other = getattr(_lib, name)
        assert not set(_lib.DBSCAN_EXPORTS) & set(other) and len(other) == length, name
    assert L.sgm_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define SGM_ABI_VERSION 4\b", txt) and "sgm_hip_dbscan.h" in txt.split("typedef enum")[0]
    assert all(callable(getattr(cv.Engine, n)) for n in ("cluster_dbscan_host", "cluster_dbscan_device"))
    assert callable(cv.cluster_dbscan) and callable(cv.largest_clusters) and {"cluster_dbscan", "largest_clusters"} <= set(cv.__all__)
    for name in NEW:      # the prototypes and the binding agree on the number of arguments
        proto = re.search(name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(getattr(L, name).argtypes) == 12
    readme = open(os.path.join(ROOT, "README.md")).read()
    for doc in (extra, cv.cluster_dbscan.__doc__, readme):
        assert re.search(r"NOT\s+Open3D", doc.replace("**", ""), flags=re.I)
    assert "cluster_dbscan" in readme and "largest_clusters" in readme
    assert "voxel_down_sample -> cluster_dbscan -> largest_clusters -> valid_points" in cv.cluster_dbscan.__doc__
    assert "ours plus\n * one" in extra or "ours plus one" in extra                # the off-by-one against Open3D's min_points
    assert _lib.DBSCAN_STAGES == ("dbscan_count", "dbscan_clear", "dbscan_insert", "dbscan_starts", "dbscan_sort", "dbscan_core",
                                  "dbscan_link", "dbscan_number", "dbscan_label")
    engine = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_engine.hip")).read()
    assert all(('"' + n + '"') in engine for n in _lib.DBSCAN_STAGES) and all(n in extra for n in _lib.DBSCAN_STAGES)
    assert cv.pointcloud.DBSCAN_STATS == DR.STATS
    dbg = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_debug.h")).read()
    assert re.search(r"SGM_DBG_DBSCAN_GATHER_CORE = 1 << 29\b", dbg) and _lib.SGM_DBG_DBSCAN_GATHER_CORE == 1 << 29
    sig = inspect.signature(cv.cluster_dbscan).parameters
    assert list(sig) == ["points_3D", "disparity_map", "eps", "min_points", "origin", "confidence", "min_confidence", "return_core",
                         "return_sizes", "return_stats"]
    assert sig["origin"].default == (0, 0, 0) and sig["confidence"].default is None and sig["min_confidence"].default == 0
    assert sig["return_core"].default is sig["return_sizes"].default is sig["return_stats"].default is False
    assert sig["eps"].default is sig["min_points"].default is inspect.Parameter.empty
    sig = inspect.signature(cv.largest_clusters).parameters
    assert list(sig) == ["labels", "sizes", "count", "min_size"] and sig["count"].default == 1 and sig["min_size"].default == 1
    makefile = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "Makefile")).read()
    assert "sgm_hip_dbscan.h" in makefile
    kernels = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "kernels_dbscan.h")).read()
    assert '#include "kernels_post.h"' in kernels and "uf_union(" in kernels and "__device__ __forceinline__ void uf_union" not in kernels


def test_the_c_entries_refuse_without_an_engine():
    """a null engine is refused before anything touches the GPU"""
    import ctypes as C
    L = _lib.load()
    org = (C.c_float * 3)(0, 0, 0)
    st = np.full(6, 7, np.uint64)
    nc = C.c_int64(-5)
    for fn in (L.sgm_cluster_dbscan, L.sgm_cluster_dbscan_device):
        assert fn(None, 8, None, 4, 0.05, 3, org, None, None, None, st.ctypes.data, C.byref(nc)) == -1   # SGM_ERR_INVALID_ARG
        assert b"sgm_cluster_dbscan" in L.sgm_last_error() and st.tolist() == [7] * 6 and nc.value == -5


@pytest.fixture()
def no_engine(monkeypatch):
    """any attempt to get an engine fails the test: the errors below are raised in front of it"""
    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(S, "get_engine", boom)
    monkeypatch.setattr(S, "Engine", boom)


def test_cluster_dbscan_argument_errors_come_before_any_engine(no_engine):
    p3, d = np.zeros((6, 9, 3), np.float32), np.ones((6, 9), np.float32)
    lst = np.zeros((10, 3), np.float32)
    cd = cv.cluster_dbscan
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        cd(p3, d[:, :8], 0.1, 4)
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        cd(lst, d, 0.1, 4)
    with pytest.raises(cv.error, match=r"\(N, 3\) list"):
        cd(p3, None, 0.1, 4)
    with pytest.raises(cv.error, match=r"\(N, 3\) list"):
        cd(np.zeros((10, 4), np.float32), None, 0.1, 4)
    with pytest.raises(cv.error, match="cluster_dbscan: points_3D must be float32"):
        cd(p3.astype(np.float64), d, 0.1, 4)
    with pytest.raises(cv.error, match="confidence must have the shape"):
        cd(p3, d, 0.1, 4, confidence=np.zeros((6, 8), np.uint8))
    with pytest.raises(cv.error, match="needs a disparity_map"):
        cd(lst, None, 0.1, 4, confidence=np.zeros(10, np.uint8))
    for k in (0, -3, 1 << 24, 1.5, True, None, "2", 2 ** 31):
        with pytest.raises(cv.error, match="min_points"):
            cd(p3, d, 0.1, k)
    for r in (0, -1.0, np.nan, np.inf, 1e-45, 1e-20, 1e20, 1e39, "x", None, (1, 2)):     # 1e-20, 1e20: the square leaves the normal range
        with pytest.raises(cv.error, match="eps"):
            cd(p3, d, r, 4)
    for o in ((0, 0), (0, 0, np.nan), (np.inf, 0, 0), 1.0, (0, 0, 0, 0), (1e39, 0, 0)):
        with pytest.raises(cv.error, match="origin"):
            cd(p3, d, 0.1, 4, origin=o)
    # an empty list needs no engine either
    out = cd(np.zeros((0, 3), np.float32), None, 0.1, 4, return_core=True, return_sizes=True, return_stats=True)
    assert out[0].shape == out[1].shape == out[2].shape == (0,) and out[0].dtype == np.int32 and out[1].dtype == np.uint8
    assert out[2].dtype == np.uint32 and out[3] == dict(in_range=0, out_of_range=0, core=0, border=0, noise=0, clusters=0)
    assert cd(np.zeros((0, 3), np.float32), None, 0.1, 4).shape == (0,)
    # the functions beside it raise what they raised
    with pytest.raises(cv.error, match="estimate_normals_radius: points_3D must be float32"):
        cv.estimate_normals_radius(p3.astype(np.float64), d, 0.1)
    with pytest.raises(cv.error, match="remove_radius_outlier: points_3D must be float32"):
        cv.remove_radius_outlier(p3.astype(np.float64), None, d, 4, 0.1)


def test_the_dbscan_kernels_use_no_scratch():
    """resource remarks of the build: every kernel of kernels_dbscan.h without scratch memory and at eight waves per SIMD"""
    txt = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "resource_usage.txt")).read()
    blocks = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", txt, flags=re.S)
    mine = {n: (int(v), int(s)) for n, v, s in blocks if "k_dbscan_" in n}
    assert len(mine) == 2 + 2 + 3, sorted(mine)                   # mark and link twice each, roots, rank, label
    assert all(s == 0 for _, s in mine.values()), mine
    assert all(v <= 64 for v, _ in mine.values()), mine
