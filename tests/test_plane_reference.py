"""Plane segmentation without a GPU: hand-worked answers of the definition (include/sgm_hip_plane.h) held against its numpy
restatement tests/plane_ref.py -- the hash, a plane from three points, the orientation rule, the emulated fused multiply-add against
exact rational arithmetic, the inclusive threshold and the refit range at their last ulp, lattices whose answer is known exactly,
the cases without a plane, what the definition promises under a reordering of the points --, the interface lists (header, binding,
library, stage names, debug bit, signatures), the refusals of the C entries without an engine, the Python argument errors, all of
which are raised before any engine exists, the scratch memory of the kernels, and the conditions on the generated clouds that keep
the GPU tests from passing on a cloud without a plane.  What the device computes is held against plane_ref.py in
tests/test_gpu_plane.py."""
import ctypes as C
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import covariance_ref as CR
import plane_ref as PR
import stereo_reconstruction_cv_amd as cv
from stereo_reconstruction_cv_amd import _lib
from stereo_reconstruction_cv_amd import stereo as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sgm_plane_inliers", "sgm_plane_inliers_device", "sgm_segment_plane", "sgm_segment_plane_device"]
F32 = np.float32


def f32(x):
    return np.asarray(x, np.float32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def exact_fma(a, b, c):
    """fma(a, b, c) of three finite binary32 numbers, correctly rounded to binary32, by exact rational arithmetic"""
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if v == 0:
        return F32(0.0) if not (np.signbit(F32(a) * F32(b)) and np.signbit(F32(c))) else F32(-0.0)
    lo = F32(float(v))                     # (float(Fraction) is correctly rounded to binary64; one of lo's neighbours is the answer)
    cands = [lo, np.nextafter(lo, F32(np.inf)), np.nextafter(lo, F32(-np.inf))]
    best = min(cands, key=lambda y: (abs(Fraction(float(y)) - v), int(F32(y).view(np.uint32)) & 1))      # nearest, ties to even
    return best


# ---- the pieces ------------------------------------------------------------------------------------------------------------------
def test_the_hash_on_three_counters_worked_by_hand():
    """step 3 in plain Python integers"""
    def by_hand(seed, c):
        M = 0xFFFFFFFF
        x = (seed ^ ((c * 0x9E3779B9) & M)) & M
        x ^= x >> 16
        x = (x * 0x7FEB352D) & M
        x ^= x >> 15
        x = (x * 0x846CA68B) & M
        x ^= x >> 16
        return x
    worked = {(0, 0): 0x0, (7, 1): 0xA715B186, (0xDEADBEEF, 12345): 0x9FA6427C}
    for (seed, c), want in worked.items():
        assert by_hand(seed, c) == want == int(PR.hash32(seed, c))
    # the rank: (x * m) >> 32, and the counters of hypothesis k are 3k, 3k + 1, 3k + 2
    assert (0xA715B186 * 1000) >> 32 == 652
    rk = PR.ranks(7, 5, 1000)
    assert rk.shape == (5, 3) and rk[0, 1] == 652 and all(int(rk[k, j]) == (by_hand(7, 3 * k + j) * 1000) >> 32 for k in range(5) for j in range(3))
    assert PR.ranks(123, 64, 1).max() == 0 and PR.ranks(123, 4096, 3).max() == 2 and PR.ranks(123, 4096, 3).min() == 0


def test_a_plane_from_three_points_by_hand():
    """step 4: (0,0,2), (1,0,2), (0,1,2) span z = 2 with n = e1 x e2 = (0,0,1), d = -2; oriented: (0,0,-1,2)"""
    P = f32([[0, 0, 2], [1, 0, 2], [0, 1, 2], [3, 0, 2]])
    planes, deg = PR.hypotheses(P, np.array([[0, 1, 2], [0, 2, 1], [0, 1, 3], [1, 1, 2]]))
    assert deg.tolist() == [False, False, True, True]                  # collinear; a point drawn twice
    assert np.array_equal(bits(planes[0]), bits([0, 0, -1, 2])) and np.array_equal(bits(planes[1]), bits([0, 0, -1, 2]))
    assert np.isnan(planes[2:]).all()
    # a tilted one: (0,0,0), (1,0,1), (0,1,0): n = (0*0 - 1*1, 1*0 - 1*0, 1*1 - 0) = (-1, 0, 1) / sqrt 2, d = 0 -> first non-zero negative: negated
    planes, deg = PR.hypotheses(f32([[0, 0, 0], [1, 0, 1], [0, 1, 0]]), np.array([[0, 1, 2]]))
    r = 1.0 / np.sqrt(2.0)
    assert not deg[0] and np.array_equal(bits(planes[0]), bits([F32(r), 0, F32(-r), 0]))


def test_orientation_and_rounding():
    """step 9: d < 0 negates; d == 0 goes by the first non-zero of a, b, c; no negative zero comes out"""
    o = PR.orient_round
    assert np.array_equal(bits(o(0.0, 0.0, 1.0, -2.0)), bits([0, 0, -1, 2]))
    assert np.array_equal(bits(o(0.0, 0.0, -1.0, 2.0)), bits([0, 0, -1, 2]))
    assert np.array_equal(bits(o(0.0, -1.0, 0.0, 0.0)), bits([0, 1, 0, 0]))
    assert np.array_equal(bits(o(0.0, 0.0, -1.0, 0.0)), bits([0, 0, 1, 0]))
    assert np.array_equal(bits(o(0.6, -0.8, 0.0, 0.0)), bits([F32(0.6), F32(-0.8), 0, 0]))
    assert np.array_equal(bits(o(-0.6, 0.8, 0.0, -0.0)), bits([F32(0.6), F32(-0.8), 0, 0]))
    assert np.array_equal(bits(o(-0.0, 1.0, -0.0, 3.0)), bits([0, 1, 0, 3]))            # the zeros lose their sign
    assert not np.signbit(o(1.0, 0.0, 0.0, -5.0)[1:3]).any()                               # ... also those a negation makes
    many = o(np.array([1.0, -1.0]), np.array([0.0, 0.0]), np.array([0.0, 0.0]), np.array([-1.0, 0.0]))
    assert np.array_equal(bits(many), bits([[-1, 0, 0, 1], [1, 0, 0, 0]]))


def test_the_emulated_fma_against_exact_arithmetic():
    """PR.fmaf equals the correctly rounded exact value on every triple of a set of awkward numbers and on random triples, and
    the triples where an unfused chain differs are among them: the test can tell the two apart"""
    small = [0.0, -0.0, 1.0, -1.0, 3.0, 1.0 / 3.0, 1 + 2.0 ** -23, 1 - 2.0 ** -24, 2.0 ** -126, 2.0 ** -149, 3 * 2.0 ** -149, 16777216.0,
             16777217.0, 0.1, -0.1, 1e-20, 1e20, 3.4028234e38, 2.0 ** -75, 1.5 * 2.0 ** -60]
    small = f32(small)
    a, b, c = (g.reshape(-1) for g in np.meshgrid(small, small, small, indexing="ij"))
    with np.errstate(all="ignore"):
        fine = np.isfinite(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))
        fine &= np.abs(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)) < 3.4e38
    a, b, c = a[fine], b[fine], c[fine]
    got = PR.fmaf(a, b, c)
    want = f32([exact_fma(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.array_equal(bits(got), bits(want))
    rng = np.random.default_rng(5)
    a, b, c = (f32(rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 4, 4000)) for _ in range(3))
    c = np.where(rng.random(4000) < 0.5, f32(-(a * b)), c)                 # heavy cancellation, where fusing matters
    got = PR.fmaf(a, b, c)
    want = f32([exact_fma(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.array_equal(bits(got), bits(want))
    with np.errstate(all="ignore"):
        unfused = f32(a * b) + c
    assert (bits(unfused) != bits(got)).sum() > 500
    # what is not finite takes the plain expression
    with np.errstate(all="ignore"):
        assert np.isnan(PR.fmaf(f32([np.inf, np.nan, 1.0]), f32([0.0, 1.0, np.inf]), f32([1.0, 1.0, -np.inf]))).all()
        assert PR.fmaf(f32([3e38]), f32([2.0]), f32([0.0]))[0] == np.inf


def test_the_threshold_is_inclusive_to_the_ulp():
    """points at exactly t and one ulp beyond on the plane z = 0"""
    t = F32(0.03)
    beyond = np.nextafter(t, F32(1))
    xyz = f32([[0, 0, t], [1, 0, -t], [0, 1, beyond], [1, 1, -beyond], [2, 2, 0]])
    got = PR.classify(xyz, None, None, f32([0, 0, 1, 0]), t, 0)
    assert got["inlier"].tolist() == [1, 1, 0, 0, 1] and got["n_inliers"] == 3 and got["index"].tolist() == [0, 1, 4]
    assert np.array_equal(bits(got["distance"]), bits([t, -t, beyond, -beyond, 0]))
    inv = PR.classify(xyz, None, None, f32([0, 0, 1, 0]), t, 1)
    assert inv["index"].tolist() == [2, 3] and np.array_equal(inv["inlier"], got["inlier"])
    # not valid: distance the quiet NaN, never selected
    xyz = f32([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0]])
    got = PR.classify(xyz, f32([1, 1, 1, 0]), None, f32([0, 0, 1, 0]), t, 1)
    assert got["inlier"].tolist() == [1, 0, 0, 0] and bits(got["distance"]).tolist() == [0] + [0x7FC00000] * 3 and got["n_selected"] == 0


def test_the_refit_range_at_its_last_ulp():
    """|u| <= 524288 is in range: with t = 32 the quantum is 1, and 524288 itself votes while the next float does not"""
    qs = PR.qscale_of(32.0)
    assert qs == 1.0
    edge = F32(524288.0)
    P = f32([[0, 0, 0], [edge, 0, 0], [np.nextafter(edge, F32(np.inf)), 0, 0], [-edge, 1, 0], [2, np.nextafter(-edge, F32(-np.inf)), 0]])
    S, m_r, oor = PR.moments(P, np.ones(5, bool), P[0], qs)
    assert (m_r, oor) == (3, 2) and S[:3] == [0, 1, 0] and S[3] == 2 * 524288 ** 2
    # the bounds of the header: |q| <= 2^19, so 2^24 terms stay below 2^43 and 2^62
    assert 524288 == 2 ** 19 and (2 ** 24 - 1) * 2 ** 38 < 2 ** 62 and (2 ** 24 - 1) * 2 ** 19 < 2 ** 43


def test_lattices_with_known_answers():
    """z = 2: the model is exactly (0, 0, -1, 2) with every point an inlier; slope 1: (1, 0, -1) / sqrt 2 within 2^-22"""
    xyz = CR.plane_lattice(12, 16)
    for refine in (False, True):
        w = PR.segment(xyz, None, None, 0.01, 64, 0, refine)
        assert np.array_equal(bits(w["model"]), bits([0, 0, -1, 2])) and w["n_inliers"] == 192 == int(w["inlier"].sum())
        assert int(w["stats"][6]) == int(refine) and int(w["stats"][7]) == 1 and int(w["stats"][3]) == 192
        assert np.array_equal(bits(w["distance"]), bits(np.zeros(192)))
    w = PR.segment(CR.plane_lattice(12, 16, slope=1.0), None, None, 0.01, 64, 0, True)
    r = 1.0 / np.sqrt(2.0)
    assert np.abs(w["model"][:3].astype(np.float64) - np.array([r, 0, -r])).max() <= 2.0 ** -22 and w["n_inliers"] == 192
    assert int(w["stats"][6]) == 1


def test_no_plane():
    """collinear points, fewer than three valid points, all-invalid input, an empty list"""
    line = f32([[k * 0.25, 1.0, 2.0] for k in range(40)])
    cases = [(line, None), (line[:2], None), (line, np.zeros(40, np.float32)), (np.full((9, 3), np.nan, np.float32), None),
             (np.zeros((0, 3), np.float32), None)]
    for xyz, disp in cases:
        w = PR.segment(xyz, disp, None, 0.01, 32, 1, True, 1)
        assert not w["model"].any() and not w["inlier"].any() and w["n_inliers"] == 0 and int(w["stats"][7]) == 0
        assert (bits(w["distance"]) == 0x7FC00000).all()
        assert w["n_selected"] == int(PR.valid_of(xyz, disp).sum())       # every valid point is "not an inlier"
    w = PR.segment(line, None, None, 0.01, 32, 1)
    assert int(w["stats"][1]) == 32 and w["stats"][2:].tolist() == [0] * 6       # every hypothesis degenerate
    assert PR.segment(line[:2], None, None, 0.01, 32, 1)["stats"].tolist() == [2, 0, 0, 0, 0, 0, 0, 0]


def test_what_holds_under_a_reordering_of_the_points():
    """The definition promises no invariance of the model under a permutation: a rank then names another point, so cnt_k, k* and
    the model may all change.  What it promises: (a) the result is self-consistent -- the mask is the classification by the
    returned model --, and (b) the counts are a function of the hypotheses alone: a permutation of the valid list that keeps the
    sampled ranks' points in place leaves every cnt_k, and with them the model, as they were."""
    xyz, disp, _ = PR.RR.layered_lists(24, 130, 724)
    a = PR.segment(xyz, disp, None, 0.03, 32, 9)
    b = PR.segment(xyz[::-1], disp[::-1], None, 0.03, 32, 9)
    for w, (p, d) in ((a, (xyz, disp)), (b, (xyz[::-1], disp[::-1]))):
        again = PR.classify(p, d, None, w["model"], 0.03, 0)
        assert np.array_equal(again["inlier"], w["inlier"]) and int(w["stats"][7]) == 1
    valid = np.nonzero(PR.valid_of(xyz, disp))[0]
    P = xyz[valid]
    keep = np.unique(a["ranks"])
    free = np.setdiff1d(np.arange(P.shape[0]), keep)
    perm = np.arange(P.shape[0])
    perm[free] = np.random.default_rng(3).permutation(free)
    c = PR.segment(P[perm], None, None, 0.03, 32, 9)
    assert np.array_equal(c["counts"], a["counts"]) and np.array_equal(bits(c["planes"]), bits(a["planes"]))
    assert np.array_equal(bits(c["model"]), bits(a["model"])) and c["n_inliers"] == a["n_inliers"]
    assert np.array_equal(c["inlier"], a["inlier"][valid][perm])


# ---- conditions on the inputs of the GPU tests -----------------------------------------------------------------------------------
def test_the_condition_cases_are_what_they_claim():
    xyz, disp, col, t, K, seed = PR.condition_case("layered")                       # (i)
    w = PR.want_of("layered", xyz, disp, col, t, K, seed)
    m, best = int(w["stats"][0]), int(w["stats"][3])
    assert 0.2 * m <= best <= 0.6 * m and int(w["stats"][6]) == 1
    assert (m, best, w["n_inliers"]) == (13576, 4942, 5093)
    xyz, disp, col, t, K, seed = PR.condition_case("tie")                           # (ii)
    w = PR.want_of("tie", xyz, disp, col, t, K, seed)
    top = np.nonzero(w["counts"] == w["counts"].max())[0]
    assert len(set(w["planes"][top][:, 3].tolist())) >= 2 and int(w["stats"][2]) == int(top[0])
    xyz, disp, col, t, K, seed = PR.condition_case("duplicates")                    # (iii)
    w = PR.want_of("duplicates", xyz, disp, col, t, K, seed)
    assert 0.1 * K <= int(w["stats"][1]) <= 0.9 * K and int(w["stats"][7]) == 1
    xyz, disp, col, t, K, seed = PR.condition_case("refit_range")                   # (iv)
    w = PR.want_of("refit_range", xyz, disp, col, t, K, seed)
    best, m_r, oor = (int(w["stats"][i]) for i in (3, 4, 5))
    assert m_r + oor == best and min(m_r, oor) >= 0.1 * best and int(w["stats"][6]) == 1
    # the shape cases: the larger ones find a plane, the smallest cannot
    for i, case in enumerate(PR.SHAPE_CASES):
        w = PR.case_want(i)
        assert int(w["stats"][7]) == (0 if case[0] == "list" and case[1] < 3 else 1), case


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; the lists fixed earlier and the ABI version stay"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "sgm_hip_plane.h")).read()
    code = re.sub(r"/\*.*?\*/", "", extra, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", code)))
    L = _lib.load()
    assert declared == sorted(_lib.PLANE_EXPORTS) == NEW
    assert '#include "sgm_hip_plane.h"' in txt and all(hasattr(L, n) for n in declared)
    assert txt.index('#include "sgm_hip_dbscan.h"') < txt.index('#include "sgm_hip_plane.h"')
    earlier = dict(EXPORTS=34, CONFIDENCE_EXPORTS=1, RIGHT_EXPORTS=1, WLS_EXPORTS=3, WLS_BATCH_EXPORTS=2, LRC_EXPORTS=3,
                   VOXEL_EXPORTS=2, MESH_EXPORTS=2, NORMALS_EXPORTS=4, RADIUS_EXPORTS=2, STATISTICAL_EXPORTS=2, COVARIANCE_EXPORTS=2,
                   DBSCAN_EXPORTS=2)
    for name, length in earlier.items():
        other = getattr(_lib, name)
        assert not set(_lib.PLANE_EXPORTS) & set(other) and len(other) == length, name
    assert L.sgm_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define SGM_ABI_VERSION 4\b", txt) and "sgm_hip_plane.h" in txt.split("typedef enum")[0]
    assert all(callable(getattr(cv.Engine, n)) for n in ("segment_plane_host", "segment_plane_device", "plane_inliers_host",
                                                         "plane_inliers_device"))
    assert callable(cv.segment_plane) and callable(cv.plane_inliers) and {"segment_plane", "plane_inliers"} <= set(cv.__all__)
    for name in NEW:      # the prototypes and the binding agree on the number of arguments
        proto = re.search(name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(getattr(L, name).argtypes) == (19 if "segment" in name else 15), name
    readme = open(os.path.join(ROOT, "README.md")).read()
    for doc in (extra, cv.segment_plane.__doc__, readme):
        assert re.search(r"NOT\s+Open3D", doc.replace("**", ""), flags=re.I)
    assert "segment_plane" in readme and "plane_inliers" in readme
    assert "segment_plane(..., invert=True) -> cluster_dbscan(confidence=mask) -> largest_clusters -> valid_points" in cv.segment_plane.__doc__
    assert "peel plane after plane" in cv.segment_plane.__doc__
    assert "the same bits come out on every run" in extra and "2^43" in extra and "2^62" in extra and "0x7FC00000" in extra
    assert _lib.PLANE_STAGES == ("plane_valid", "plane_sample", "plane_count", "plane_best", "plane_moments", "plane_solve", "plane_classify",
                                 "plane_compact")
    engine = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_engine.hip")).read()
    assert all(('"' + n + '"') in engine for n in _lib.PLANE_STAGES) and all(n in extra for n in _lib.PLANE_STAGES)
    assert cv.pointcloud.PLANE_STATS == PR.STATS
    dbg = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_debug.h")).read()
    assert re.search(r"SGM_DBG_PLANE_OTHER_COUNT = 1 << 30\b", dbg) and _lib.SGM_DBG_PLANE_OTHER_COUNT == 1 << 30
    sig = inspect.signature(cv.segment_plane).parameters
    assert list(sig) == ["points_3D", "colors", "disparity_map", "distance_threshold", "ransac_n", "num_iterations", "seed", "refine",
                         "invert", "confidence", "min_confidence", "return_points", "return_index", "return_distances", "return_stats"]
    assert (sig["ransac_n"].default, sig["num_iterations"].default, sig["seed"].default) == (3, 1000, 0)
    assert sig["refine"].default is True and sig["invert"].default is False and sig["confidence"].default is None
    assert sig["min_confidence"].default == 0 and sig["distance_threshold"].default is inspect.Parameter.empty
    assert all(sig[n].default is False for n in ("return_points", "return_index", "return_distances", "return_stats"))
    sig = inspect.signature(cv.plane_inliers).parameters
    assert list(sig)[:6] == ["points_3D", "colors", "disparity_map", "plane_model", "distance_threshold", "invert"]
    makefile = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "Makefile")).read()
    assert "sgm_hip_plane.h" in makefile
    kernels = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "kernels_plane.h")).read()
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in kernels and "cov_normal(" in kernels and "__builtin_fmaf" in kernels
    asm = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_engine.s")).read()
    assert "v_mfma_f32_16x16x4_f32" in asm or "v_mfma_f32_16x16x4f32" in asm


def test_the_c_entries_refuse_without_an_engine():
    """a null engine is refused before anything touches the GPU, with every output untouched"""
    L = _lib.load()
    model = np.full(4, 7, np.float32)
    st = np.full(8, 7, np.uint64)
    ni, ns = C.c_int64(-5), C.c_int64(-6)
    for fn in (L.sgm_segment_plane, L.sgm_segment_plane_device):
        rc = fn(None, 8, None, None, 4, 0.05, 16, 0, 1, 0, None, None, None, None, None, model.ctypes.data, st.ctypes.data, C.byref(ni), C.byref(ns))
        assert rc == -1 and b"sgm_segment_plane" in L.sgm_last_error()      # SGM_ERR_INVALID_ARG
        assert model.tolist() == [7] * 4 and st.tolist() == [7] * 8 and (ni.value, ns.value) == (-5, -6)
    unit = np.array([0, 0, 1, 0], np.float32)
    for fn in (L.sgm_plane_inliers, L.sgm_plane_inliers_device):
        rc = fn(None, 8, None, None, 4, unit.ctypes.data, 0.05, 0, None, None, None, None, None, C.byref(ni), C.byref(ns))
        assert rc == -1 and b"sgm_plane_inliers" in L.sgm_last_error() and (ni.value, ns.value) == (-5, -6)


@pytest.fixture()
def no_engine(monkeypatch):
    """any attempt to get an engine fails the test: the errors below are raised in front of it"""
    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(S, "get_engine", boom)
    monkeypatch.setattr(S, "Engine", boom)


def test_argument_errors_come_before_any_engine(no_engine):
    p3, d = np.zeros((6, 9, 3), np.float32), np.ones((6, 9), np.float32)
    lst = np.zeros((10, 3), np.float32)
    sp, pi = cv.segment_plane, cv.plane_inliers
    unit = (0, 0, 1, 0)
    for call in (lambda *a, **k: sp(a[0], a[1], a[2], 0.1, **k), lambda *a, **k: pi(a[0], a[1], a[2], unit, 0.1, **k)):
        with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
            call(p3, None, d[:, :8])
        with pytest.raises(cv.error, match=r"\(N, 3\) list"):
            call(p3, None, None)
        with pytest.raises(cv.error, match="points_3D must be float32"):
            call(p3.astype(np.float64), None, d)
        with pytest.raises(cv.error, match="colors must be uint8"):
            call(p3, np.zeros((6, 9, 3), np.float32), d)
        with pytest.raises(cv.error, match="confidence must have the shape"):
            call(p3, None, d, confidence=np.zeros((6, 8), np.uint8))
        with pytest.raises(cv.error, match="needs a disparity_map"):
            call(lst, None, None, confidence=np.zeros(10, np.uint8))
    for t in (0, -1.0, np.nan, np.inf, 1e-45, 1e-39, 1e39, "x", None, (1, 2)):      # 1e-39: not a normal number
        with pytest.raises(cv.error, match="distance_threshold"):
            sp(p3, None, d, t)
        with pytest.raises(cv.error, match="distance_threshold"):
            pi(p3, None, d, unit, t)
    for r in (1, 2, 4, 3.0, True, None):
        with pytest.raises(cv.error, match="ransac_n"):
            sp(p3, None, d, 0.1, ransac_n=r)
    for k in (0, -3, 65537, 1.5, True, None, "2"):
        with pytest.raises(cv.error, match="num_iterations"):
            sp(p3, None, d, 0.1, num_iterations=k)
    for s in (-1, 2 ** 32, 1.5, True, None):
        with pytest.raises(cv.error, match="seed"):
            sp(p3, None, d, 0.1, seed=s)
    for m in ((0, 0, 1), (0, 0, 2, 0), (0, 0, np.nan, 0), (0, 0, 1, np.inf), (0, 0, 1.002, 0), (0, 0, 0, 0), "abcd", None):
        with pytest.raises(cv.error, match="plane_model"):
            pi(p3, None, d, m, 0.1)
    # an empty list needs no engine either
    out = sp(np.zeros((0, 3), np.float32), None, None, 0.1, return_points=True, return_index=True, return_distances=True, return_stats=True)
    model, mask, pts, col, idx, dist, st = out
    assert model.tolist() == [0, 0, 0, 0] and mask.shape == (0,) and mask.dtype == np.uint8 and pts.shape == (0, 3) and col is None
    assert idx.shape == (0,) and idx.dtype == np.uint32 and dist.shape == (0,) and st == dict(zip(PR.STATS, [0] * 8))
    assert pi(np.zeros((0, 3), np.float32), None, None, unit, 0.1).shape == (0,)
    assert pi(np.zeros((0, 3), np.float32), None, None, (0, 0, 1.0004, 0), 0.1, invert=True).shape == (0,)      # squared: within 2^-10 of 1
    # the functions beside it raise what they raised
    with pytest.raises(cv.error, match="cluster_dbscan: points_3D must be float32"):
        cv.cluster_dbscan(p3.astype(np.float64), d, 0.1, 4)


def test_the_plane_kernels_use_no_scratch():
    """resource remarks of the build: every kernel of kernels_plane.h without scratch memory"""
    txt = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "resource_usage.txt")).read()
    blocks = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", txt, flags=re.S)
    mine = {n: (int(v), int(s)) for n, v, s in blocks if "k_plane_" in n}
    assert len(mine) == 9, sorted(mine)       # valid_count, valid_scatter, sample, count_valu, count_mfma, best, moments, solve, classify
    assert all(s == 0 for _, s in mine.values()), mine
