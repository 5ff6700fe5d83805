"""Rigid registration without a GPU: hand-worked answers of the definition (include/sgm_hip_icp.h) held against its numpy restatement
tests/icp_ref.py -- the tie rule, the inclusive radius at its last ulp, an unplaced point, an unusable normal, the tree and its
padding, the quaternion update, the evaluation alone --, the correspondence over all pairs against the 27 cells on the case table,
sgm_icp_solve of the library against the reference's solve and update bit for bit, the interface lists (header, binding, library,
stage names, signatures), the refusals of the C entries without an engine, the Python argument errors, all of which are raised before
any engine exists, the scratch memory of the kernels, the conditions on the generated clouds that keep the GPU tests from passing on
clouds that exercise nothing, and the recovery of a known motion.  What the device computes is held against icp_ref.py in
tests/test_gpu_icp.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import icp_ref as IR
import radius_ref as RR
import stereo_reconstruction_cv_amd as cv
from stereo_reconstruction_cv_amd import _lib
from stereo_reconstruction_cv_amd import stereo as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = sorted(["sgm_register_icp", "sgm_register_icp_device", "sgm_evaluate_registration", "sgm_evaluate_registration_device",
              "sgm_transform_points", "sgm_transform_points_device", "sgm_icp_solve"])
F32, F64 = np.float32, np.float64
EYE = np.eye(4)
DEBUG_BITS = 9      # the `SGM_DBG_... = 1 << k` enumerators of csrc/sgm_debug.h before this call existed: it added none


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def f32(x):
    return np.asarray(x, np.float32).reshape(-1, 3)


# ---- the pieces ------------------------------------------------------------------------------------------------------------------
def test_a_tie_goes_to_the_lower_target_index():
    """one source point, two targets at binary32-equal distances, in both orders"""
    src = f32([[1.0, 2.0, 3.0]])
    for tgt in (f32([[1.25, 2, 3], [0.75, 2, 3]]), f32([[0.75, 2, 3], [1.25, 2, 3]])):
        cl = IR.Clouds(src, None, tgt, None, None, 0.5)
        for how in ("brute", "cells"):
            ev = IR.evaluate(cl, EYE, 0, how)
            assert ev["corr"].tolist() == [0] and ev["d2"].tolist() == [0.0625] and ev["fitness"] == 1.0 and ev["rmse"] == 0.25
    # a nearer target at a higher index still wins
    ev = IR.evaluate(IR.Clouds(src, None, f32([[1.25, 2, 3], [0.75, 2, 3], [1.125, 2, 3]]), None, None, 0.5), EYE)
    assert ev["corr"].tolist() == [2]


def test_the_radius_is_inclusive_to_the_last_ulp():
    """a target exactly at r (d2 == r2) is a partner, one ulp beyond is not"""
    r = F32(0.25)
    src = f32([[0, 0, 0], [0, 4, 0]])
    beyond = np.nextafter(r, F32(1))
    tgt = f32([[r, 0, 0], [beyond, 4, 0]])
    assert F32(beyond) * F32(beyond) > r * r
    for how in ("brute", "cells"):
        ev = IR.evaluate(IR.Clouds(src, None, tgt, None, None, r), EYE, 0, how)
        assert ev["corr"].tolist() == [0, -1] and u32(ev["d2"]).tolist() == [int(u32(r * r)[0]), 0x7FC00000]
        assert ev["fitness"] == 0.5 and ev["rmse"] == 0.25


def test_an_unplaced_point_and_the_counts():
    """a transformation that takes a valid source point out of the grid's range or to infinity: no partner, counted; points that
    are not valid are in no count"""
    src = f32([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [2, 0, 0]])
    disp = np.array([1, 1, 1, 0], F32)
    tgt = f32([[0, 0, 0.0625], [1, 0, 0.0625]])
    cl = IR.Clouds(src, disp, tgt, None, None, 0.125)
    assert cl.m_s == 2
    ev = IR.evaluate(cl, EYE)
    assert ev["corr"].tolist() == [0, 1, -1, -1] and ev["unplaced"] == 0 and ev["fitness"] == 1.0
    T = EYE.copy()
    T[0, 0] = 1.0e5                                  # x = 1 goes to 1e5: cell index 775 757, out of range
    ev = IR.evaluate(cl, T)
    assert ev["corr"].tolist() == [0, -1, -1, -1] and ev["unplaced"] == 1 and ev["fitness"] == 0.5
    T[0, 3] = 1.0e39                                 # rounds to infinity in binary32: nobody is placed
    ev = IR.evaluate(cl, T)
    assert ev["unplaced"] == 2 and ev["n_corr"] == 0 and ev["fitness"] == 0.0 and ev["rmse"] == 0.0 and not ev["sums"].any()


def test_an_unusable_normal_counts_but_does_not_vote():
    src = f32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]])
    tgt = src + F32(0.0625)
    nrm = f32([[0, 0, 1], [0, 0, 0], [0, 0.499, 0], [np.nan, 0, 1]])          # unit; zero; squared length under 0.25; not finite
    cl = IR.Clouds(src, None, tgt, None, nrm, 0.25)
    ev = IR.evaluate(cl, EYE, 1)
    assert ev["unusable"] == 3 and ev["n_corr"] == 4 and ev["fitness"] == 1.0
    # only point 0 votes: a = (0, 0, 0, 0, 0, 1), e = d_z = -0.0625
    want = np.zeros(28)
    want[20] = 1.0
    want[26] = 0.0625
    want[27] = 4 * 3 * 0.0625 ** 2
    assert u64(ev["sums"] + 0.0).tolist() == u64(want).tolist()
    assert IR.usable_normals(f32([[0, 0, 0.5], [0, 0, 2], [0, 0, 2.001], [0.5, 0, 0]])).tolist() == [True, True, False, True]


def test_the_tree_and_its_padding():
    """ns = 1, 2, 3 by hand, the order of a larger tree against sequential summation, and the zero of an empty tail"""
    assert IR.tree(np.array([[5.0]]))[0] == 5.0
    assert u64(IR.tree(np.array([[-0.0]]))).tolist() == u64([-0.0]).tolist()           # one term: no addition at all
    assert u64(IR.tree(np.array([[-0.0], [-0.0], [-0.0]]))).tolist() == u64([0.0]).tolist()   # (-0 + -0) + (-0 + +0) = +0
    a, b, c = 1.0, 2.0 ** -53, 2.0 ** -53
    assert IR.tree(np.array([[a], [b], [c]]))[0] == (a + b) + (c + 0.0) == 1.0
    assert IR.tree(np.array([[b], [c], [a]]))[0] == (b + c) + (a + 0.0) == 1.0 + 2.0 ** -52
    v = np.random.default_rng(3).standard_normal(11)
    by_hand = (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))) + (((v[8] + v[9]) + (v[10] + 0.0)) + ((0.0 + 0.0) + (0.0 + 0.0)))
    assert IR.tree(v.reshape(-1, 1))[0] == by_hand
    # point-to-point terms of one pair by hand
    src, tgt = f32([[1, 2, 3]]), f32([[1.5, 2.25, 2.875]])
    ev = IR.evaluate(IR.Clouds(src, None, tgt, None, None, 1.0), EYE, 0)
    d = (-0.5, -0.25, 0.125)
    want = [13, -2, -3, 0, -3, 2, 10, -6, 3, 0, -1, 5, -2, 1, 0, 1, 0, 0, 1, 0, 1,
            -(2 * d[2] - 3 * d[1]), -(3 * d[0] - 1 * d[2]), -(1 * d[1] - 2 * d[0]), 0.5, 0.25, -0.125, 0.25 + 0.0625 + 0.015625]
    assert (ev["sums"] == np.array(want)).all()


def test_the_quaternion_update_is_a_rotation_to_rounding():
    """R R^T - I of step 7's matrix, measured over random steps up to a radian: a few ulp, with no sin, cos or sqrt"""
    rng = np.random.default_rng(9)
    worst = 0.0
    for _ in range(300):
        x = list(rng.uniform(-1, 1, 3)) + [0.0, 0.0, 0.0]
        R = np.array(IR.rotation_of(x))
        worst = max(worst, float(np.abs(R @ R.T - np.eye(3)).max()), abs(float(np.linalg.det(R)) - 1.0))
    print("orthogonality error of the quaternion update:", worst)
    assert worst < 8 * np.finfo(np.float64).eps
    # a quarter turn about z is exact: the quaternion (1, 0, 0, 1)
    assert np.array(IR.rotation_of([0, 0, 2.0, 0, 0, 0])).tolist() == [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T = IR.update([0, 0, 2.0, 1, 2, 3], EYE)
    assert T.tolist() == [[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]]


def test_no_iterations_is_the_evaluation():
    src, ds, tgt, dt, tn = IR.case_input(IR.SHAPE_CASES.index((257, 300)))
    T0 = IR.rigid((0, 0, 1), 0.5, (0.01, 0, 0))
    w = IR.register(src, ds, tgt, dt, tn, IR.R_CASE, T0=T0, estimation=1, max_iteration=0)
    ev = IR.evaluate(IR.Clouds(src, ds, tgt, dt, tn, IR.R_CASE), T0, 0)
    assert u64(w["T"]).tolist() == u64(T0).tolist() and w["history"].shape == (1, 2) and int(w["stats"][3]) == 0
    assert (w["fitness"], w["rmse"]) == (ev["fitness"], ev["rmse"]) == tuple(w["history"][0])
    assert (w["corr"] == ev["corr"]).all() and (u32(w["d2"]) == u32(ev["d2"])).all() and int(w["stats"][7]) == IR.MAX_ITER
    # an empty source, an empty target
    w = IR.register(np.zeros((0, 3), F32), None, tgt, dt, tn, IR.R_CASE, T0=T0)
    assert w["stats"].tolist() == [0, 0, 0, 0, 0, 0, 0, 2] and w["fitness"] == 0 and u64(w["T"]).tolist() == u64(T0).tolist()
    w = IR.register(src, ds, np.zeros((0, 3), F32), None, np.zeros((0, 3), F32), IR.R_CASE, T0=T0)
    assert int(w["stats"][7]) == IR.TOO_FEW and int(w["stats"][0]) > 0 and (w["corr"] == -1).all() and w["fitness"] == 0


@pytest.mark.parametrize("i", range(len(IR.SHAPE_CASES)))
def test_all_pairs_and_27_cells_agree(i):
    """the lemma at work for a query point that is not a record of the grid: both statements of step 3 give the same pairs"""
    ns, nt = IR.SHAPE_CASES[i]
    src, ds, tgt, dt, tn = IR.case_input(i)
    cl = IR.Clouds(src, ds, tgt, dt, tn, IR.R_CASE)
    for T in (EYE, IR.rigid((1, 1, 0), 1.5, (0.02, 0.0, -0.02))):
        P = IR.transform(IR.m_of(T), cl.src)
        placed, g = IR.placed_of(P, cl.valid, cl.r, cl.origin)
        if ns > 1000:          # (all pairs of the largest source: a strided sample of it)
            placed = placed & (np.arange(ns) % 16 == 3)
        a = IR.correspond_brute(P, placed, cl.tgt, cl.q_in, cl.r)
        b = IR.correspond_cells(P, placed, g, cl.tgt, cl.q_in, cl.gq, cl.r)
        assert (a[0] == b[0]).all() and (u32(a[1]) == u32(b[1])).all()
        assert ns < 63 or nt < 300 or (a[0] >= 0).sum() > 0.2 * placed.sum()


# ---- sgm_icp_solve ---------------------------------------------------------------------------------------------------------------
def lib_solve(sums, T, estimation=1, in_place=False):
    L = _lib.load()
    sums = np.ascontiguousarray(sums, F64)
    Tin = np.ascontiguousarray(T, F64).reshape(16).copy()
    Tout = Tin if in_place else np.full(16, 7.0)
    st = C.c_int(-9)
    assert L.sgm_icp_solve(sums.ctypes.data, estimation, Tin.ctypes.data, Tout.ctypes.data, C.byref(st)) == 0
    return Tout.reshape(4, 4), st.value


def test_the_library_solve_equals_the_reference_bit_for_bit():
    """steps 6 and 7 on the host: sums from the case table under both estimations, an identity system, a singular one"""
    T0 = IR.rigid((2, -1, 1), 3.0, (0.1, 0.2, -0.3))
    n = 0
    for i, (ns, nt) in enumerate(IR.SHAPE_CASES):
        if ns < 63 or ns > 1000 or nt < 300:
            continue
        src, ds, tgt, dt, tn = IR.case_input(i)
        cl = IR.Clouds(src, ds, tgt, dt, tn, IR.R_CASE)
        for est in (0, 1):
            sums = IR.evaluate(cl, EYE, est)["sums"]
            want, st = IR.solve_update(sums, T0)
            got, gst = lib_solve(sums, T0, est)
            assert st == gst and u64(got).tolist() == u64(want).tolist(), (ns, nt, est)
            assert u64(lib_solve(sums, T0, est, in_place=True)[0]).tolist() == u64(want).tolist()
            n += st == 0
    assert n >= 8
    ident = np.zeros(28)
    ident[[0, 6, 11, 15, 18, 20]] = 1.0
    ident[21:27] = [0.0, 0.0, 2.0, 1.0, 2.0, 3.0]
    got, st = lib_solve(ident, EYE)
    assert st == 0 and got.tolist() == [[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]]
    assert u64(IR.solve_update(ident, T0)[0]).tolist() == u64(lib_solve(ident, T0)[0]).tolist()
    singular = ident.copy()
    singular[11] = 0.0
    for bad in (singular, -ident, np.full(28, np.nan), np.where(np.arange(28) == 0, np.inf, ident)):
        got, st = lib_solve(bad, T0)
        assert st == 3 == IR.solve_update(bad, T0)[1] and u64(got).tolist() == u64(T0).tolist()
    L = _lib.load()
    st = C.c_int(-9)
    assert L.sgm_icp_solve(None, 0, None, None, C.byref(st)) == -1 and st.value == -9 and b"sgm_icp_solve" in L.sgm_last_error()
    t = np.eye(4).reshape(16)
    assert L.sgm_icp_solve(ident.ctypes.data, 2, t.ctypes.data, t.ctypes.data, C.byref(st)) == -1 and st.value == -9


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; the lists fixed earlier and the ABI version stay"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "sgm_hip_icp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", extra, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", code)))
    L = _lib.load()
    assert declared == sorted(_lib.ICP_EXPORTS) == NEW
    assert '#include "sgm_hip_icp.h"' in txt and all(hasattr(L, n) for n in declared)
    assert txt.index('#include "sgm_hip_plane.h"') < txt.index('#include "sgm_hip_icp.h"')
    earlier = dict(EXPORTS=34, CONFIDENCE_EXPORTS=1, RIGHT_EXPORTS=1, WLS_EXPORTS=3, WLS_BATCH_EXPORTS=2, LRC_EXPORTS=3,
                   VOXEL_EXPORTS=2, MESH_EXPORTS=2, NORMALS_EXPORTS=4, RADIUS_EXPORTS=2, STATISTICAL_EXPORTS=2, COVARIANCE_EXPORTS=2,
                   DBSCAN_EXPORTS=2, PLANE_EXPORTS=4)
    for name, length in earlier.items():
        other = getattr(_lib, name)
        assert not set(_lib.ICP_EXPORTS) & set(other) and len(other) == length, name
    assert L.sgm_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define SGM_ABI_VERSION 4\b", txt) and "sgm_hip_icp.h" in txt.split("typedef enum")[0]
    assert all(callable(getattr(cv.Engine, n)) for n in ("register_icp_host", "register_icp_device", "evaluate_registration_host",
                                                         "evaluate_registration_device", "transform_points_host",
                                                         "transform_points_device"))
    names = {"registration_icp", "evaluate_registration", "transform_points"}
    assert all(callable(getattr(cv, n)) for n in names) and names <= set(cv.__all__)
    counts = dict(sgm_register_icp=22, sgm_register_icp_device=22, sgm_evaluate_registration=15, sgm_evaluate_registration_device=15,
                  sgm_transform_points=7, sgm_transform_points_device=7, sgm_icp_solve=5)
    for name in NEW:      # the prototypes and the binding agree on the number of arguments
        proto = re.search(r"\b" + name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(getattr(L, name).argtypes) == counts[name], name
    readme = open(os.path.join(ROOT, "README.md")).read()
    for doc in (extra, cv.registration_icp.__doc__, cv.evaluate_registration.__doc__, readme.split("registration_icp", 1)[1]):
        assert re.search(r"NOT\s+Open3D", doc.replace("**", ""), flags=re.I)
    for doc in (extra, cv.registration_icp.__doc__):      # ... and why
        for why in ("tie rule", "range rule", "Umeyama", "quaternion", "Euler", "tree"):
            assert why in doc, why
    assert all(n in readme for n in names)
    assert ("voxel_down_sample -> estimate_normals_radius (target) -> registration_icp -> transform_points -> concatenate -> write_ply"
            in cv.registration_icp.__doc__)
    assert "the same bits come out on every run" in extra and "0x7FC00000" in extra and "27 cells" in extra and "232-byte" in extra
    assert _lib.ICP_STAGES == ("icp_count", "icp_clear", "icp_insert", "icp_starts", "icp_sort", "icp_correspond", "icp_terms", "icp_reduce")
    engine = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_engine.hip")).read()
    assert all(('"' + n + '"') in engine for n in _lib.ICP_STAGES) and all(n in extra for n in _lib.ICP_STAGES)
    assert cv.pointcloud.ICP_STATS == IR.STATS and cv.pointcloud.ICP_MAX_ITERATION == IR.MAX_ITERATION
    dbg = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_debug.h")).read()
    assert not re.search(r"SGM_DBG_ICP", dbg) and len(re.findall(r"\bSGM_DBG_[A-Z0-9_]+\s*=\s*1\s*<<", dbg)) == DEBUG_BITS      # no debug bit was added
    sig = inspect.signature(cv.registration_icp).parameters
    assert list(sig) == ["source", "target", "max_correspondence_distance", "init", "estimation", "target_normals", "source_disparity",
                         "target_disparity", "max_iteration", "relative_fitness", "relative_rmse", "origin", "return_correspondences",
                         "return_history", "return_stats"]
    assert (sig["init"].default, sig["estimation"].default, sig["max_iteration"].default) == (None, "point_to_plane", 30)
    assert (sig["relative_fitness"].default, sig["relative_rmse"].default, sig["origin"].default) == (1e-6, 1e-6, (0, 0, 0))
    assert all(sig[n].default is False for n in ("return_correspondences", "return_history", "return_stats"))
    sig = inspect.signature(cv.evaluate_registration).parameters
    assert list(sig)[:4] == ["source", "target", "max_correspondence_distance", "transformation"] and sig["transformation"].default is None
    assert list(inspect.signature(cv.transform_points).parameters) == ["points", "transformation", "normals"]
    makefile = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "Makefile")).read()
    assert "sgm_hip_icp.h" in makefile
    kernels = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "kernels_icp.h")).read()
    assert "rad_walk(" in kernels and "__builtin_fmaf" in kernels and "atomicAdd(&ctl" in kernels and "__shfl_down" in kernels
    assert "&e->icp_corr, &e->icp_d2, &e->icp_part" in engine      # sgm_trim gives them back


def test_the_c_entries_refuse_without_an_engine():
    """a null engine is refused before anything touches the GPU, with every output untouched"""
    L = _lib.load()
    T = np.full(16, 7.0)
    st = np.full(8, 7, np.uint64)
    hist = np.full(62, 7.0)
    fit, rmse = C.c_double(-5.0), C.c_double(-6.0)
    org = np.zeros(3, F32)
    T0 = np.eye(4).reshape(16)
    for fn in (L.sgm_register_icp, L.sgm_register_icp_device):
        rc = fn(None, 8, None, 4, 8, None, None, 4, 0.05, org.ctypes.data, T0.ctypes.data, 0, 30, 1e-6, 1e-6, T.ctypes.data, C.byref(fit),
                C.byref(rmse), None, None, hist.ctypes.data, st.ctypes.data)
        assert rc == -1 and b"sgm_register_icp" in L.sgm_last_error()      # SGM_ERR_INVALID_ARG
        assert T.tolist() == [7] * 16 and st.tolist() == [7] * 8 and hist.tolist() == [7] * 62 and (fit.value, rmse.value) == (-5, -6)
    for fn in (L.sgm_evaluate_registration, L.sgm_evaluate_registration_device):
        rc = fn(None, 8, None, 4, 8, None, 4, 0.05, org.ctypes.data, T0.ctypes.data, C.byref(fit), C.byref(rmse), None, None, st.ctypes.data)
        assert rc == -1 and b"sgm_evaluate_registration" in L.sgm_last_error()
        assert st.tolist() == [7] * 8 and (fit.value, rmse.value) == (-5, -6)
    for fn in (L.sgm_transform_points, L.sgm_transform_points_device):
        assert fn(None, 8, None, 4, T0.ctypes.data, 8, None) == -1 and b"sgm_transform_points" in L.sgm_last_error()


@pytest.fixture()
def no_engine(monkeypatch):
    """any attempt to get an engine fails the test: the errors below are raised in front of it"""
    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(S, "get_engine", boom)
    monkeypatch.setattr(S, "Engine", boom)


def test_argument_errors_come_before_any_engine(no_engine):
    lst = np.zeros((10, 3), F32)
    img, d = np.zeros((6, 9, 3), F32), np.ones((6, 9), F32)
    nrm = np.zeros((10, 3), F32)
    icp, ev, tp = cv.registration_icp, cv.evaluate_registration, cv.transform_points
    for call in (lambda s, t, **k: icp(s, t, 0.1, estimation="point_to_point", **k), lambda s, t, **k: ev(s, t, 0.1, **k)):
        with pytest.raises(cv.error, match=r"\(N, 3\) list"):
            call(img, lst)
        with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
            call(lst, img, target_disparity=d[:, :8])
        with pytest.raises(cv.error, match="must be float32"):
            call(lst.astype(np.float64), lst)
        with pytest.raises(cv.error, match="source_disparity must be float32"):
            call(img, lst, source_disparity=d.astype(np.float64))
    for r in (0, -1.0, np.nan, np.inf, 1e-30, 1e30, "x", None, (1, 2)):
        with pytest.raises(cv.error, match="max_correspondence_distance"):
            icp(lst, lst, r, estimation="point_to_point")
        with pytest.raises(cv.error, match="max_correspondence_distance"):
            ev(lst, lst, r)
    bad_T = (np.eye(3), np.full((4, 4), np.nan), np.diag([1.0, 1, 1, 2]), np.ones((4, 4)), "abcd", [1, 2, 3])
    for T in bad_T:
        with pytest.raises(cv.error, match="init"):
            icp(lst, lst, 0.1, init=T, estimation="point_to_point")
        with pytest.raises(cv.error, match="transformation"):
            ev(lst, lst, 0.1, transformation=T)
        with pytest.raises(cv.error, match="transformation"):
            tp(lst, T)
    with pytest.raises(cv.error, match="transformation"):
        tp(lst, None)
    for est in ("plane", 0, 1, None, "POINT_TO_PLANE"):
        with pytest.raises(cv.error, match="estimation"):
            icp(lst, lst, 0.1, estimation=est, target_normals=nrm)
    with pytest.raises(cv.error, match="needs target_normals"):
        icp(lst, lst, 0.1)
    with pytest.raises(cv.error, match="target_normals must be float32"):
        icp(lst, lst, 0.1, target_normals=nrm[:9])
    for k in (-1, 1001, 1.5, True, None, "2"):
        with pytest.raises(cv.error, match="max_iteration"):
            icp(lst, lst, 0.1, estimation="point_to_point", max_iteration=k)
    for v in (-1e-9, np.nan, "x", None, True):
        with pytest.raises(cv.error, match="relative_fitness"):
            icp(lst, lst, 0.1, estimation="point_to_point", relative_fitness=v)
        with pytest.raises(cv.error, match="relative_rmse"):
            icp(lst, lst, 0.1, estimation="point_to_point", relative_rmse=v)
    with pytest.raises(cv.error, match="origin"):
        icp(lst, lst, 0.1, estimation="point_to_point", origin=(0, np.inf, 0))
    with pytest.raises(cv.error, match=r"points must be float32 \(\.\.\., 3\)"):
        tp(np.zeros((4, 2), F32), np.eye(4))
    with pytest.raises(cv.error, match="normals must be float32"):
        tp(lst, np.eye(4), normals=nrm[:3])
    # an empty source needs no engine either
    T0 = IR.rigid((0, 0, 1), 10, (1, 2, 3))
    T, fit, rmse, corr, d2, hist, st = icp(np.zeros((0, 3), F32), lst, 0.1, init=T0, estimation="point_to_point",
                                           return_correspondences=True, return_history=True, return_stats=True)
    assert u64(T).tolist() == u64(T0).tolist() and (fit, rmse) == (0.0, 0.0) and corr.shape == (0,) and corr.dtype == np.int32
    assert d2.shape == (0,) and hist.tolist() == [[0, 0]] and st == dict(zip(IR.STATS, [0] * 7 + ["too_few"]))
    assert ev(np.zeros((0, 3), F32), lst, 0.1) == (0.0, 0.0)
    assert tp(np.zeros((0, 3), F32), np.eye(4)).shape == (0, 3)
    # the functions beside it raise what they raised
    with pytest.raises(cv.error, match="segment_plane: points_3D must be float32"):
        cv.segment_plane(img.astype(np.float64), None, d, 0.1)


def test_the_icp_kernels_use_no_scratch():
    """resource remarks of the build: every kernel of kernels_icp.h without scratch memory"""
    txt = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "resource_usage.txt")).read()
    blocks = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", txt, flags=re.S)
    mine = {n: (int(v), int(s)) for n, v, s in blocks if "k_icp_" in n}
    assert len(mine) == 4, sorted(mine)       # correspond, terms, reduce, transform
    for name, (vgprs, scratch) in mine.items():
        assert scratch == 0 and vgprs <= 128, (name, vgprs, scratch)


# ---- the conditions on the generated cases ------------------------------------------------------------------------------------------
def test_the_generated_cases_exercise_what_they_claim():
    src, ds, tgt, dt, tn, r = IR.condition_case("layered")
    cl = IR.Clouds(src, ds, tgt, dt, tn, r)
    ev = IR.evaluate(cl, EYE, 1)
    none = cl.m_s - ev["n_corr"] - ev["unplaced"]
    assert min(ev["n_corr"], ev["unplaced"], none) >= 0.1 * cl.m_s and ev["unusable"] >= 0.03 * ev["n_corr"]
    assert cl.t_in < cl.tgt.shape[0] and cl.m_s < cl.src.shape[0]
    src, _, tgt, _, _, r = IR.condition_case("tie")
    d = RR.d2_of(src[:, None, :], tgt.reshape(300, 2, 3))
    assert (u32(d[:, 0]) == u32(d[:, 1])).all() and (d[:, 0] <= RR.constants(r)[0]).all()
    ev = IR.evaluate(IR.Clouds(src, None, tgt, None, None, r), EYE)
    assert ev["corr"].tolist() == [2 * k for k in range(300)]
    assert (tgt[0::2, 0] > src[:, 0])[0::2].all() and (tgt[0::2, 0] < src[:, 0])[1::2].all()      # the winner is on either side in turn
    src, _, tgt, _, tn, r = IR.condition_case("plane")
    w = IR.register(src, None, tgt, None, tn, r, estimation=1)
    assert int(w["stats"][7]) == IR.DEGENERATE and int(w["stats"][4]) == 192 and int(w["stats"][3]) == 0
    assert int(IR.register(src, None, tgt, None, tn, r, estimation=0, max_iteration=3)["stats"][7]) != IR.DEGENERATE
    src, _, tgt, _, tn, r = IR.condition_case("corner")
    for est in (0, 1):
        ev = IR.evaluate(IR.Clouds(src, None, tgt, None, tn, r), EYE, est)
        A = np.zeros((6, 6))
        A[np.triu_indices(6)] = ev["sums"][:21]
        A = A + np.triu(A, 1).T
        assert np.linalg.matrix_rank(A) == 6 and np.linalg.cond(A) < 1e6 and IR.solve(ev["sums"]) is not None
    # every shape case that can has correspondences, and the table reaches three of the four statuses
    seen = set()
    for i, (ns, nt) in enumerate(IR.SHAPE_CASES):
        if ns > 1000:
            continue
        w = IR.case_want(i, True, 1)
        seen.add(int(w["stats"][7]))
        assert ns < 63 or nt < 300 or int(w["stats"][4]) >= 6, (ns, nt)
    assert {IR.MAX_ITER, IR.TOO_FEW} <= seen


# ---- recovery ----------------------------------------------------------------------------------------------------------------------
# measured on the reference (this file, CPU) with the default thresholds: the sine of the rotation error and the translation error
# of the recovered motion.  Point-to-point converges after 10 iterations, point-to-plane after 4; the rmse ends at the binary32
# rounding of the copy, 6e-8.  (With both thresholds 0 the call runs all 30 iterations and the rmse wanders between 5.5e-8 and
# 7.0e-8 from the 10th on: at that floor the history is NOT monotone, which is why the thresholds of this test are the defaults.)
RECOVERY_MEASURED = dict(point_to_point=(1.1823211538933686e-08, 3.0559972593438113e-08),
                         point_to_plane=(4.370007937445606e-09, 1.8102819434041985e-08))
RECOVERY_BOUND = 4 * 3.0559972593438113e-08      # 4 times the larger measured value: the case is seeded, not adversarial


def motion_error(T, truth):
    E = np.asarray(T) @ np.linalg.inv(truth)
    ang = float(np.linalg.norm([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])) / 2.0      # sin of the angle: arccos is blind here
    return ang, float(np.linalg.norm(np.asarray(T)[:3, 3] - truth[:3, 3]))


def recovery_want(est):
    src, tgt, tn, truth = IR.recovery_case()
    return IR.shared(("recovery", est), lambda: IR.register(src, None, tgt, None, tn, IR.R_CASE, estimation=est, max_iteration=30)), truth


@pytest.mark.parametrize("est", (0, 1))
def test_a_known_motion_is_recovered(est):
    """the target is a rigid copy of the source (2 degrees about an oblique axis, a translation of about half of r): the
    reference's motion against the known one, within 4 times the larger error measured on this seeded case; its rmse never rises"""
    w, truth = recovery_want(est)
    ang, tr = motion_error(w["T"], truth)
    print("recovery", ("point_to_point", "point_to_plane")[est], "rotation error", ang, "translation error", tr, "rmse", w["rmse"],
          "fitness", w["fitness"], "iterations", int(w["stats"][3]))
    assert max(ang, tr) <= RECOVERY_BOUND
    h = w["history"][:, 1]
    assert (h[1:] <= h[:-1]).all() and w["fitness"] == 1.0 and int(w["stats"][7]) == IR.CONVERGED
    assert 2 <= int(w["stats"][3]) <= 20      # (measured: 10 and 4; the generator goes through libm, so the count is not held exactly)
