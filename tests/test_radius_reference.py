"""Radius outlier removal without a GPU: hand-worked answers of the definition (include/sgm_hip_radius.h) held against its numpy
restatement tests/radius_ref.py, the two forms of the reference against each other, the symmetry of the neighbour relation, the
saturation, the range rule, the header's lemma measured over all pairs, the interface lists (header, binding, library, ABI
version) and the Python argument errors, all of which are raised before any engine exists.  What the device computes is held
against radius_ref.py in tests/test_gpu_radius.py."""
import inspect
import os
import re

import numpy as np
import pytest

import radius_ref as RR
import voxel_ref as VR
import stereo_reconstruction_cv_amd as cv
from stereo_reconstruction_cv_amd import _lib
from stereo_reconstruction_cv_amd import stereo as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sgm_radius_outlier", "sgm_radius_outlier_device"]
F32 = np.float32


def f32(x):
    return np.asarray(x, np.float32)


def same(a, b):
    for k in ("keep", "counts", "index", "full", "in_range"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["points"].view(np.uint32), b["points"].view(np.uint32))
    assert (a["colors"] is None) == (b["colors"] is None) and (a["colors"] is None or np.array_equal(a["colors"], b["colors"]))
    assert (a["n_kept"], a["n_out_of_range"]) == (b["n_kept"], b["n_out_of_range"])


def both(xyz, disp=None, colors=None, **kw):
    a, b = RR.brute(f32(xyz), disp, colors, **kw), RR.cells(f32(xyz), disp, colors, **kw)
    same(a, b)
    return a


# ---- the definition, by hand -----------------------------------------------------------------------------------------------------
def test_two_points_at_exactly_r_count_and_one_ulp_beyond_do_not():
    """r = 0.25, coordinates multiples of 0.25: dx = 0.25 exactly, d2 = 0.0625 = r2, and the test is inclusive"""
    r = both([[0.5, 0.75, 1.0], [0.75, 0.75, 1.0]], radius=0.25, nb_points=1)
    assert r["full"].tolist() == [1, 1] and r["keep"].tolist() == [1, 1] and r["n_kept"] == 2
    beyond = np.nextafter(F32(0.75), F32(1))
    assert beyond - F32(0.5) > F32(0.25)                      # the difference is representable: one ulp of 0.75 more than r
    r = both([[0.5, 0.75, 1.0], [beyond, 0.75, 1.0]], radius=0.25, nb_points=1)
    assert r["full"].tolist() == [0, 0] and r["n_kept"] == 0 and r["points"].shape == (0, 3)
    # along a diagonal: (0.25, 0.25, 0) is 0.3536 away, outside; r = 0.5: d2 = 0.125 <= 0.25, inside
    assert both([[0, 0, 0], [0.25, 0.25, 0]], radius=0.25, nb_points=1)["full"].tolist() == [0, 0]
    assert both([[0, 0, 0], [0.25, 0.25, 0]], radius=0.5, nb_points=1)["full"].tolist() == [1, 1]


def test_duplicates_count_and_a_point_does_not_count_itself():
    pts = [[1, 2, 3]] * 4 + [[9, 9, 9]]
    r = both(pts, colors=np.arange(15, dtype=np.uint8).reshape(5, 3), radius=0.125, nb_points=3)
    assert r["full"].tolist() == [3, 3, 3, 3, 0] and r["keep"].tolist() == [1, 1, 1, 1, 0]
    assert r["index"].tolist() == [0, 1, 2, 3] and r["colors"].tolist() == np.arange(12).reshape(4, 3).tolist()
    assert both(pts, radius=0.125, nb_points=4)["n_kept"] == 0
    assert both([[1, 2, 3]], radius=0.125, nb_points=1)["full"].tolist() == [0]


def test_validity_is_the_voxel_grid_s():
    pts = f32([[0, 0, 0], [0.1, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0.1, 0], [0, 0, 0.1]])
    disp = f32([1, 1, 1, 1, 0, -1])
    r = both(pts, disp, radius=0.5, nb_points=1)
    assert r["in_range"].tolist() == [True, True, False, False, False, False] and r["full"].tolist() == [1, 1, 0, 0, 0, 0]
    assert both(pts, None, radius=0.5, nb_points=1)["full"].tolist() == [3, 3, 0, 0, 3, 3]
    assert r["n_out_of_range"] == 0


def test_saturation_at_max_count():
    xyz, disp, col = RR.layered_lists(24, 130, 724)
    full = both(xyz, disp, col, radius=0.03, nb_points=4, max_count=RR.FULL)
    assert full["full"].max() > 12 and np.array_equal(full["counts"], full["full"])
    for mc in (4, 7):
        r = both(xyz, disp, col, radius=0.03, nb_points=4, max_count=mc)
        assert np.array_equal(r["counts"], np.minimum(full["full"], mc)) and (r["counts"] == mc).sum() > 100
        assert np.array_equal(r["keep"], full["keep"]) and np.array_equal(r["keep"], r["counts"] >= 4)
    assert np.array_equal(both(xyz, disp, col, radius=0.03, nb_points=4)["counts"], np.minimum(full["full"], 4))     # None: nb_points


def test_the_range_rule_at_plus_and_minus_2_to_the_16():
    r = F32(1.0)
    _, v, inv = RR.constants(r)
    edge = F32(65536.0) * v                      # exact: v = 1.03125
    assert np.floor(edge * inv) == 65536.0 and np.floor(np.nextafter(edge, F32(0)) * inv) == 65535.0
    assert np.floor(-edge * inv) == -65536.0 and np.floor(np.nextafter(-edge, F32(-1e9)) * inv) == -65537.0
    inside_hi, inside_lo = np.nextafter(edge, F32(0)), -edge
    pts = f32([[inside_hi, 0, 0], [edge, 0, 0], [inside_lo, 0, 0], [np.nextafter(-edge, F32(-1e9)), 0, 0],
               [0, inside_hi, 0], [0, 0, edge], [3e38, 0, 0]])
    res = both(pts, radius=r, nb_points=1)
    assert res["in_range"].tolist() == [True, False, True, False, True, False, False] and res["n_out_of_range"] == 4
    # the points out of range are nobody's neighbour, although they sit an ulp from one that is in range
    assert res["full"].tolist() == [0] * 7 and res["keep"].tolist() == [0] * 7
    twin = np.concatenate([pts, pts])
    assert both(twin, radius=r, nb_points=1)["full"].tolist() == [1, 0, 1, 0, 1, 0, 0] * 2
    # a non-zero origin moves the range with it
    res = both(pts + f32([[100, 0, 0]]), radius=r, nb_points=1, origin=(100, 0, 0))
    assert res["in_range"].tolist()[:4] == [True, False, True, False]


def test_neighbour_cells_outside_the_range_are_skipped():
    """a point in the last cell of the range: its neighbour cells at index 2^16 do not exist, the others do"""
    r = F32(1.0)
    _, v, _ = RR.constants(r)
    last = F32(65535.5) * v
    pts = f32([[last, last, last], [last - F32(0.5), last, last], [-last, -last, -last], [-last + F32(0.5), -last, -last]])
    assert both(pts, radius=r, nb_points=1)["full"].tolist() == [1, 1, 1, 1]


# ---- the two forms, and the properties ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(RR.SHAPE_CASES)))
def test_the_two_forms_agree_on_the_case_table(i):
    kind, a, b, r, nb, mc, o = RR.SHAPE_CASES[i]
    xyz, disp, col = RR.case_input(i)
    same(RR.brute(xyz, disp, col, r, nb, mc, o), RR.case_want(i))
    if kind == "layered" and a == 24:       # (the all-pairs form takes two seconds on the larger cloud: once is enough there)
        same(RR.brute(xyz, None, col, r, nb, mc, o), RR.case_want(i, with_disp=False))


def test_the_case_table_exercises_both_branches():
    """every shape of the issue is in the table, and the (r, nb) pairs of the 48 x 320 cloud keep the fractions it states"""
    shapes = [c[1] if c[0] == "list" else c[1:3] for c in RR.SHAPE_CASES]
    assert shapes[:6] == [1, 2, 63, 64, 65, 257] and (24, 130) in shapes and (48, 320) in shapes
    xyz, disp, col = RR.layered_lists(48, 320, 704)
    for (r, nb), frac in (((0.02, 8), 0.67), ((0.02, 16), 0.44), ((0.01, 4), 0.31)):
        res = RR.cells(xyz, disp, None, r, nb)
        nvalid = int(res["in_range"].sum())
        assert nvalid == 13576 and abs(res["n_kept"] / nvalid - frac) < 0.006, (r, nb, res["n_kept"] / nvalid)
    for i in range(6, len(RR.SHAPE_CASES)):
        w = RR.case_want(i)
        assert 0.05 < w["n_kept"] / w["in_range"].sum() < 0.95


def test_the_neighbour_relation_is_symmetric():
    xyz, _ = RR.random_list(700, 11, 0.5)
    xyz = xyz[np.isfinite(xyz).all(axis=1)]
    r2, _, _ = RR.constants(0.06)
    near = RR.d2_of(xyz[:, None, :], xyz[None, :, :]) <= r2
    assert np.array_equal(near, near.T) and near.sum() > 3 * xyz.shape[0]
    assert np.array_equal(RR.brute(xyz, radius=0.06, nb_points=1)["full"], near.sum(axis=1) - 1)
    # reversing the cloud reverses the counts: nothing depends on the order of the points
    a, b = RR.cells(xyz, radius=0.06, nb_points=2, max_count=RR.FULL), RR.cells(xyz[::-1].copy(), radius=0.06, nb_points=2, max_count=RR.FULL)
    assert np.array_equal(a["counts"], b["counts"][::-1])


def test_pairs_across_every_face_edge_and_corner():
    for origin in ((0.0, 0.0, 0.0), (0.3, -1.7, 2.2)):
        xyz, dirs = RR.face_pairs(0.25, origin)
        res = both(xyz, radius=0.25, nb_points=1, origin=origin)
        assert res["full"].tolist() == [1] * 52 and len(dirs) == 26
        _, _, g = RR.classify(xyz, None, 0.25, origin)
        assert np.array_equal(g[1::2] - g[0::2], dirs)           # each pair does straddle what it is named for


def test_the_exact_lattice_in_closed_form():
    xyz, nb = RR.lattice(6, 0.25, (-0.5, 0.25, 1.0))
    res = both(xyz, radius=0.25, nb_points=6, max_count=RR.FULL)
    assert np.array_equal(res["full"], 6 - nb) and sorted(set(res["full"].tolist())) == [3, 4, 5, 6]
    assert res["n_kept"] == 4 ** 3
    xyz, _ = RR.lattice(6, 0.75)
    assert both(xyz, radius=0.25, nb_points=1)["full"].max() == 0


# ---- the lemma of the header ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0.005, 0.01, 0.02, 0.04])
def test_no_pair_within_r_is_more_than_one_cell_apart_on_the_layered_cloud(r):
    xyz, disp, _ = RR.layered_lists(48, 320, 704)
    ok = np.isfinite(xyz).all(axis=1) & (disp > 0)
    assert RR.max_cell_difference(xyz[ok], r) == 1


def test_no_pair_within_r_is_more_than_one_cell_apart_near_cell_faces():
    """points within an ulp of cell faces, where the rounding of t decides the cell, at small and at the largest indices, with
    partners at distances within an ulp of r"""
    rng = np.random.default_rng(5)
    for r, span in ((0.25, 40), (0.0371, 40), (1.0, 65000), (3.3e-3, 65000), (0.7, 9)):
        _, v, _ = RR.constants(r)
        for origin in ((0.0, 0.0, 0.0), (0.37, -11.1, 5.0e-3)):
            k = rng.integers(-span, span, size=(300, 3)).astype(np.float64)
            face = (k * float(v) + np.asarray(origin)).astype(np.float32)
            ulps = rng.integers(-2, 3, size=face.shape)
            a = face.copy()
            for s in (-2, -1, 1, 2):
                a = np.where(ulps == s, np.nextafter(np.nextafter(a, F32(np.sign(s) * 3e38)), F32(np.sign(s) * 3e38)) if abs(s) == 2
                             else np.nextafter(a, F32(np.sign(s) * 3e38)), a)
            d = rng.normal(size=(300, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            scale = float(r) * (1 + rng.integers(-3, 4, size=(300, 1)) * 2.0 ** -23)
            b = (a.astype(np.float64) + d * scale).astype(np.float32)
            axis = (np.eye(3)[rng.integers(0, 3, size=300)] * rng.choice([-1.0, 1.0], size=(300, 1)))
            c = (a.astype(np.float64) + axis * scale).astype(np.float32)
            pts = np.concatenate([a, b, c])
            worst = RR.max_cell_difference(pts, r, origin)
            assert worst in (0, 1), (r, origin, worst)
    assert worst == 1


def test_no_pair_within_r_is_more_than_one_cell_apart_on_random_clouds():
    for seed, r in ((1, 0.05), (2, 0.11), (3, 0.31)):
        xyz, _ = RR.random_list(1500, seed, 1.0)
        assert RR.max_cell_difference(xyz[np.isfinite(xyz).all(axis=1)], r, (0.01, 0.02, -0.03)) == 1


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; the lists fixed earlier and the ABI version stay"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "sgm_hip_radius.h")).read()
    code = re.sub(r"/\*.*?\*/", "", extra, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", code)))
    L = _lib.load()
    assert declared == sorted(_lib.RADIUS_EXPORTS) == NEW
    assert '#include "sgm_hip_radius.h"' in txt and all(hasattr(L, n) for n in declared)
    assert txt.index('#include "sgm_hip_normals.h"') < txt.index('#include "sgm_hip_radius.h"')
    for other in (_lib.EXPORTS, _lib.CONFIDENCE_EXPORTS, _lib.RIGHT_EXPORTS, _lib.WLS_EXPORTS, _lib.WLS_BATCH_EXPORTS, _lib.LRC_EXPORTS,
                  _lib.VOXEL_EXPORTS, _lib.MESH_EXPORTS, _lib.NORMALS_EXPORTS):
        assert not set(_lib.RADIUS_EXPORTS) & set(other)
    assert L.sgm_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define SGM_ABI_VERSION 4\b", txt) and "sgm_hip_radius.h" in txt.split("typedef enum")[0]
    assert all(callable(getattr(cv.Engine, n)) for n in ("radius_outlier_host", "radius_outlier_device"))
    assert callable(cv.remove_radius_outlier) and "remove_radius_outlier" in cv.__all__
    for name in NEW:      # the prototypes and the binding agree on the number of arguments
        proto = re.search(name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(getattr(L, name).argtypes) == 16
    for doc in (extra, cv.remove_radius_outlier.__doc__, open(os.path.join(ROOT, "README.md")).read()):
        assert re.search(r"NOT\s+Open3D", doc.replace("**", ""), flags=re.I)
    for doc in (extra, cv.remove_radius_outlier.__doc__, open(os.path.join(ROOT, "README.md")).read(),
                open(os.path.join(ROOT, "DESIGN.md")).read()):
        assert re.search(r"thins\s+the\s+far\s+range", doc)
    dbg = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_debug.h")).read()
    assert re.search(r"SGM_DBG_RADIUS_TIGHT_TABLE = 1 << 24\b", dbg) and re.search(r"SGM_DBG_RADIUS_SOURCE_ORDER = 1 << 25\b", dbg)
    assert (_lib.SGM_DBG_RADIUS_TIGHT_TABLE, _lib.SGM_DBG_RADIUS_SOURCE_ORDER) == (1 << 24, 1 << 25)
    assert RR.MAX_POINTS == cv.pointcloud.RADIUS_MAX_POINTS == (1 << 24) - 1 >= 4096 * 2160
    assert list(inspect.signature(cv.remove_radius_outlier).parameters) == [
        "points_3D", "colors", "disparity_map", "nb_points", "radius", "origin", "max_count", "confidence", "min_confidence",
        "return_mask", "return_counts", "return_index"]


def test_the_c_entries_refuse_without_an_engine():
    """a null engine is refused before anything touches the GPU"""
    import ctypes as C
    L = _lib.load()
    org = (C.c_float * 3)(0, 0, 0)
    nk = C.c_int64(-7)
    for fn in (L.sgm_radius_outlier, L.sgm_radius_outlier_device):
        assert fn(None, 8, None, None, 4, 0.05, org, 1, 1, None, None, 16, None, None, C.byref(nk), None) == -1   # SGM_ERR_INVALID_ARG
        assert b"sgm_radius_outlier" in L.sgm_last_error() and nk.value == -7


@pytest.fixture()
def no_engine(monkeypatch):
    """any attempt to get an engine fails the test: the errors below are raised in front of it"""
    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(S, "get_engine", boom)
    monkeypatch.setattr(S, "Engine", boom)


def test_remove_radius_outlier_argument_errors_come_before_any_engine(no_engine):
    p3, d, c = np.zeros((6, 9, 3), np.float32), np.ones((6, 9), np.float32), np.zeros((6, 9, 3), np.uint8)
    lst = np.zeros((10, 3), np.float32)
    rro = cv.remove_radius_outlier
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        rro(p3, c, d[:, :8], 4, 0.1)
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        rro(lst, None, d, 4, 0.1)
    with pytest.raises(cv.error, match=r"\(N, 3\) list"):
        rro(p3, c, None, 4, 0.1)
    with pytest.raises(cv.error, match=r"\(N, 3\) list"):
        rro(np.zeros((10, 4), np.float32), None, None, 4, 0.1)
    with pytest.raises(cv.error, match="float32"):
        rro(p3.astype(np.float64), c, d, 4, 0.1)
    for bad in (c[:5], c.astype(np.float32)):
        with pytest.raises(cv.error, match="colors must be uint8"):
            rro(p3, bad, d, 4, 0.1)
    with pytest.raises(cv.error, match="colors must be uint8"):
        rro(lst, np.zeros((9, 3), np.uint8), None, 4, 0.1)
    with pytest.raises(cv.error, match="confidence must have the shape"):
        rro(p3, c, d, 4, 0.1, confidence=np.zeros((6, 8), np.uint8))
    with pytest.raises(cv.error, match="needs a disparity_map"):
        rro(lst, None, None, 4, 0.1, confidence=np.zeros(10, np.uint8))
    for r in (0, -1.0, np.nan, np.inf, 1e-45, 1e-20, 1e20, 1e39, "x", None, (1, 2)):     # 1e-20, 1e20: the square leaves the normal range
        with pytest.raises(cv.error, match="radius"):
            rro(p3, c, d, 4, r)
    for o in ((0, 0), (0, 0, np.nan), (np.inf, 0, 0), 1.0, (0, 0, 0, 0), (1e39, 0, 0)):
        with pytest.raises(cv.error, match="origin"):
            rro(p3, c, d, 4, 0.1, origin=o)
    for nb in (0, -3, 1.5, True, None, "2", 2 ** 31):
        with pytest.raises(cv.error, match="nb_points"):
            rro(p3, c, d, nb, 0.1)
    for mc in (3, 0, -1, 1.5, True, "9", 2 ** 31):
        with pytest.raises(cv.error, match="max_count"):
            rro(p3, c, d, 4, 0.1, max_count=mc)
    # an empty list needs no engine either
    out = rro(np.zeros((0, 3), np.float32), None, None, 4, 0.1, return_mask=True, return_counts=True, return_index=True)
    assert out[0].shape == (0, 3) and out[1] is None and [a.shape for a in out[2:]] == [(0,)] * 3


def test_the_outlier_searches_keep_their_registers_on_the_shared_walk():
    """resource remarks of the build: k_radius_query and k_stat_query, whose loop over the 27 cells is rad_walk with their own
    state in a predicate and a visitor, without scratch memory and at no fewer waves per SIMD than with the loop written out in
    each (8 for both orders of k_radius_query; 8, 8, 5, 4 for the lists of 8, 16, 32 and 64 words of k_stat_query)"""
    txt = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "resource_usage.txt")).read()
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", txt, flags=re.S)
    mine = {n: (int(s), int(o)) for n, s, o in blocks if "k_radius_query" in n or "k_stat_query" in n}
    floor = {"k_radius_queryILb1E": 8, "k_radius_queryILb0E": 8, "k_stat_queryILi8E": 8, "k_stat_queryILi16E": 8, "k_stat_queryILi32E": 5,
             "k_stat_queryILi64E": 4}
    assert len(mine) == len(floor), sorted(mine)
    for key, waves in floor.items():
        (scratch, occupancy), = [v for n, v in mine.items() if key in n]
        assert scratch == 0 and occupancy >= waves, (key, scratch, occupancy)
