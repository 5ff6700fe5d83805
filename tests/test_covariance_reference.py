"""Covariance normals without a GPU: hand-worked answers of the definition (include/sgm_hip_covariance.h) held against its numpy
restatement tests/covariance_ref.py, the two forms of the reference against each other, the invariances under the order of the
points and under a power-of-two scale, the bound on the quantised offsets measured, the Jacobi solver against LAPACK, what the
quantisation costs against an unquantised binary64 PCA, the interface lists (header, binding, library, stage names), the Python
argument errors, all of which are raised before any engine exists, and the scratch memory of the two kernels.  What the device
computes is held against covariance_ref.py in tests/test_gpu_covariance.py."""
import inspect
import os
import re

import numpy as np
import pytest

import covariance_ref as CR
import stereo_reconstruction_cv_amd as cv
from stereo_reconstruction_cv_amd import _lib
from stereo_reconstruction_cv_amd import stereo as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sgm_covariance_normals", "sgm_covariance_normals_device"]
F32 = np.float32
NCASE = len(CR.SHAPE_CASES)


def f32(x):
    return np.asarray(x, np.float32)


def same(a, b):
    for k in ("counts", "stats", "moments", "has_normal", "degenerate", "in_range"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("normals", "curvature"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def both(xyz, disp=None, **kw):
    a, b = CR.brute(f32(xyz), disp, **kw), CR.cells(f32(xyz), disp, **kw)
    same(a, b)
    return a


def stats(r):
    return dict(zip(CR.STATS, (int(x) for x in r["stats"])))


# ---- the definition, by hand -----------------------------------------------------------------------------------------------------
PTS3 = [[0, 0, 0], [0.5, 0, 0], [0, 0.25, 0]]


def test_a_point_with_two_neighbours_by_hand():
    """r = 1: qscale = 2^15 and every offset quantises exactly.  The point at the origin has the neighbours (0.5, 0, 0) and
    (0, 0.25, 0): q = (2^14, 0, 0) and (0, 2^13, 0), so S = (2^14, 2^13, 0), S_00 = 2^28, S_11 = 2^26 and the other four are 0;
    m = 3.  C_00 = 2^28 - 2^28 / 3, C_01 = -2^27 / 3, C_11 = 2^26 - 2^26 / 3, and the row and column of z are 0: only the rotation
    (0, 1) ever runs, the smallest diagonal entry is a_22 = 0 exactly, the normal is (0, 0, 1) as the rotations leave it and
    kappa is 0.  Seen from (0, 0, 5) it stays, seen from (0, 0, -5) it turns."""
    r = both(PTS3, radius=1.0, min_neighbors=2, viewpoint=(0, 0, 5))
    assert r["counts"].tolist() == [2, 2, 2] and stats(r) == dict(in_range=3, out_of_range=0, with_normal=3, degenerate=0)
    assert r["moments"][0].tolist() == [1 << 14, 1 << 13, 0, 1 << 28, 0, 0, 1 << 26, 0, 0]
    C, A = CR.covariance(r["moments"][0], 3)
    assert C == [2.0 ** 28 - 2.0 ** 28 / 3.0, 0.0 - 2.0 ** 27 / 3.0, 0.0, 2.0 ** 26 - 2.0 ** 26 / 3.0, 0.0, 0.0]
    assert A[0] == 1.0 and A[1] == C[1] / C[0] and A[3] == C[3] / C[0] and A[2] == A[4] == A[5] == 0.0
    lam, V, off = CR.jacobi(A)
    assert off == [0.0, 0.0, 0.0] and lam[2] == 0.0 and min(lam[0], lam[1]) > 0.1 and [V[0][2], V[1][2], V[2][2]] == [0.0, 0.0, 1.0]
    assert abs(lam[0] + lam[1] - (A[0] + A[3])) < 1e-15                       # the trace
    assert (r["normals"] == f32([0, 0, 1])).all() and (r["curvature"] == 0).all()
    r = both(PTS3, radius=1.0, min_neighbors=2, viewpoint=(0, 0, -5))
    assert (r["normals"] == f32([0, 0, -1])).all()
    r = both(PTS3, radius=1.0, min_neighbors=2, orient=False)
    assert (r["normals"] == f32([0, 0, 1])).all()
    # the other two points: the offsets of point 1 are (-2^14, 0, 0) and (-2^14, 2^13, 0)
    assert r["moments"][1].tolist() == [-(1 << 15), 1 << 13, 0, 1 << 29, -(1 << 27), 0, 1 << 26, 0, 0]


def test_exactly_k_and_k_minus_1_neighbours():
    r = both(PTS3, radius=1.0, min_neighbors=2)
    assert r["has_normal"].all()
    r = both(PTS3, radius=1.0, min_neighbors=3)
    assert not r["has_normal"].any() and (r["normals"] == 0).all() and (r["curvature"] == -1).all() and r["counts"].tolist() == [2, 2, 2]
    assert stats(r) == dict(in_range=3, out_of_range=0, with_normal=0, degenerate=0)
    pts = PTS3 + [[0, 0, 0.78]]                # the last point is within 0.8 of the origin only
    r = both(pts, radius=0.8, min_neighbors=3)
    assert r["counts"].tolist() == [3, 2, 2, 1] and r["has_normal"].tolist() == [True, False, False, False]


def test_a_neighbour_at_exactly_r_and_one_ulp_beyond():
    far = np.nextafter(F32(0.5), F32(1))
    pts = f32([[0, 0, 0], [0.5, 0, 0], [0, far, 0], [0, 0, -0.5]])
    r = both(pts, radius=0.5, min_neighbors=2)
    assert r["counts"].tolist() == [2, 1, 0, 1]                              # 0.5 is in (d2 == r2), the next float is out
    assert r["moments"][0].tolist() == [1 << 15, 0, -(1 << 15), 1 << 30, 0, 0, 0, 0, 1 << 30]
    assert (np.abs(r["normals"][0]) == f32([0, 1, 0])).all() and r["curvature"][0] == 0


def test_duplicates_of_the_query_point_only_are_degenerate():
    pts = np.tile(f32([[0.3, -0.2, 1.7]]), (5, 1))
    r = both(pts, radius=0.1, min_neighbors=2)
    assert r["counts"].tolist() == [4] * 5 and r["degenerate"].all() and not r["has_normal"].any()
    assert (r["normals"] == 0).all() and (r["curvature"] == -1).all() and (r["moments"] == 0).all()
    assert stats(r) == dict(in_range=5, out_of_range=0, with_normal=0, degenerate=5)


def test_collinear_neighbours_give_the_tie_to_the_lowest_index():
    """three points on the x axis: C has C_00 only, the diagonal is (1, 0, 0), the two zeros tie and index 1 wins"""
    pts = [[-0.25, 0, 0], [0, 0, 0], [0.25, 0, 0]]
    r = both(pts, radius=1.0, min_neighbors=2, orient=False)
    assert (r["normals"] == f32([0, 1, 0])).all() and (r["curvature"] == 0).all()
    r = both(f32(pts)[:, [2, 0, 1]], radius=1.0, min_neighbors=2, orient=False)          # on the y axis: (1, 0, 0)
    assert (r["normals"] == f32([1, 0, 0])).all()


def test_the_exact_plane_z_const():
    """a 9 x 9 lattice of spacing 0.25 at Z = 2 with r = 0.5: qscale = 2^16, every offset is a multiple of 2^14.  No z offset,
    so the row and column of z stay 0 and the normal is column 2 of the identity: (0, 0, 1), turned to (0, 0, -1) by a viewpoint at
    the origin; kappa is exactly 0.  An interior point has 12 neighbours: 4 at 0.25, 4 at 0.3536, 4 at exactly 0.5."""
    P = CR.plane_lattice(9, 9)
    r = both(P, radius=0.5, min_neighbors=3)
    assert r["has_normal"].all() and (r["normals"] == f32([0, 0, -1])).all() and (r["curvature"] == 0).all()
    assert r["counts"].reshape(9, 9)[2:7, 2:7].tolist() == [[12] * 5] * 5 and r["counts"][0] == 5
    assert (r["moments"][:, :3] % (1 << 14) == 0).all() and r["moments"][40].tolist() == [0, 0, 0, 14 << 28, 0, 0, 14 << 28, 0, 0]
    r = both(P, radius=0.5, min_neighbors=3, orient=False)
    assert (r["normals"] == f32([0, 0, 1])).all()
    r = both(P, radius=0.5, min_neighbors=3, viewpoint=(0, 0, 10))
    assert (r["normals"] == f32([0, 0, 1])).all()


def test_the_plane_z_equals_x():
    """the same lattice tilted by 45 degrees about y: the normal is (1, 0, -1) / sqrt 2 towards the origin"""
    P = CR.plane_lattice(9, 9, slope=1.0)
    r = both(P, radius=0.5, min_neighbors=3)
    h = F32(1 / np.sqrt(2))
    inner = np.zeros((9, 9), bool)
    inner[2:7, 2:7] = True
    assert r["has_normal"].all() and (r["normals"][inner.reshape(-1)] == f32([h, 0, -h])).all()
    # at the rim the neighbourhood is lopsided and all three rotations run: the last bit of a component may differ, and the
    # smallest eigenvalue is 0 up to the roundings of the rotations, a few 2^-53 of the largest, which is 1
    assert np.abs(r["normals"] - f32([h, 0, -h])).max() <= 2.0 ** -23 and (r["curvature"] >= 0).all() and (r["curvature"] < 1e-15).all()


# ---- the two forms, the invariances, the bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NCASE))
def test_the_two_forms_agree_on_the_case_table(i):
    r, k, o, w, orient = CR.SHAPE_CASES[i][3:]
    xyz, disp = CR.case_input(i)
    want = CR.case_want(i)
    same(CR.brute(xyz, disp, r, k, o, w, bool(orient)), want)
    if xyz.shape[0] >= 63:
        assert want["has_normal"].sum() > 0.2 * xyz.shape[0], stats(want)


def test_reversing_the_points_changes_nothing():
    for i in (2, 7, 8):
        r, k, o, w, orient = CR.SHAPE_CASES[i][3:]
        xyz, disp = CR.case_input(i)
        back = CR.cells(np.ascontiguousarray(xyz[::-1]), None if disp is None else disp[::-1].copy(), r, k, o, w, bool(orient))
        want = CR.case_want(i)
        for key in ("normals", "curvature", "counts"):
            assert np.array_equal(back[key][::-1].view(np.uint32), want[key].view(np.uint32)), (i, key)
        assert np.array_equal(back["moments"][::-1], want["moments"]) and back["stats"].tolist() == want["stats"].tolist()


@pytest.mark.parametrize("e", [10, -10, 40, -40])
def test_scaling_by_a_power_of_two_changes_nothing(e):
    s = F32(2.0) ** e
    for i in (2, 7):
        r, k, o, w, orient = CR.SHAPE_CASES[i][3:]
        xyz, _ = CR.case_input(i)
        got = CR.cells(xyz * s, None, F32(r) * s, k, f32(o) * s, f32(w) * s, bool(orient))
        same(got, CR.case_want(i, with_disp=False) if CR.case_input(i)[1] is not None else CR.case_want(i))


def test_the_bound_on_the_quantised_offsets():
    """|q_a| <= 2^15 + 1 over all pairs: random lists at several radii, and neighbours at exactly r along an axis"""
    top = -1
    for seed, r in ((3, 0.1), (4, 0.3), (5, 0.7), (6, 1e-3), (7, 37.5)):
        xyz, _ = CR.random_list(400, seed, 0.5 if r < 1 else 200.0)
        if r == 1e-3:
            xyz = (xyz * F32(0.01)).astype(np.float32)
        top = max(top, CR.max_abs_q(np.ascontiguousarray(xyz[np.isfinite(xyz).all(axis=1)]), r))
    for r in (0.1, 0.3, 1.0, 3.0, 0.7):
        top = max(top, CR.max_abs_q(f32([[0, 0, 0], [r, 0, 0], [0, -F32(r), 0]]), r))
    print("largest |q_a|:", top)
    assert (1 << 15) - 2 <= top <= (1 << 15) + 1, top


# ---- the solver against LAPACK, the quantisation against binary64 ------------------------------------------------------------------------
def neighbourhoods():
    """(S, c) of every point with a normal of the case table, and 150 each of planar, linear and isotropic synthetic ones"""
    out = []
    for i in range(NCASE):
        w = CR.case_want(i)
        out += [(tuple(int(x) for x in w["moments"][j]), int(w["counts"][j])) for j in np.nonzero(w["has_normal"])[0]]
    rng = np.random.default_rng(5)
    for kind in ("planar", "linear", "isotropic"):
        for _ in range(150):
            n = int(rng.integers(4, 60))
            d = rng.normal(size=(n, 3)) * 0.3
            if kind == "planar":
                d[:, 2] *= 1e-3
            if kind == "linear":
                d[:, 1:] *= 1e-3
            q = np.rint(np.clip(d, -1, 1) * 16384).astype(np.int64)
            out.append((tuple(int(x) for x in q.sum(axis=0)) + tuple(int((q[:, a] * q[:, b]).sum()) for a, b in CR.PAIRS), n))
    return out


# four times the largest values the reference shows over neighbourhoods() (measured: 1.33e-15, 3.43e-16, 3.69e-16)
EIG_BOUND, RESIDUAL_BOUND, SINE_GAP_BOUND = 5.4e-15, 1.4e-15, 1.5e-15


def test_the_jacobi_sweeps_against_lapack():
    e_l = e_r = e_s = e_off = 0.0
    N = neighbourhoods()
    assert len(N) > 2000
    for S_, c in N:
        _, A = CR.covariance(S_, c + 1)
        lam, V, off = CR.jacobi(A)
        M = np.array([[A[0], A[1], A[2]], [A[1], A[3], A[4]], [A[2], A[4], A[5]]])
        w, U = np.linalg.eigh(M)
        e_l = max(e_l, float(np.abs(np.sort(lam) - w).max()))
        i = int(np.argmin(lam))
        nv = np.array([V[0][i], V[1][i], V[2][i]])
        e_r = max(e_r, float(np.abs(M @ nv - lam[i] * nv).max()))
        sine = np.linalg.norm(np.cross(nv, U[:, 0])) / (np.linalg.norm(nv) * np.linalg.norm(U[:, 0]))
        e_s = max(e_s, float(sine * (w[1] - w[0])))
        e_off = max(e_off, max(abs(x) for x in off))
    print(f"eigenvalues {e_l:.3g}, residual {e_r:.3g}, sine x gap {e_s:.3g}, off-diagonal {e_off:.3g} over {len(N)} neighbourhoods")
    assert e_off == 0.0 and e_l <= EIG_BOUND and e_r <= RESIDUAL_BOUND and e_s <= SINE_GAP_BOUND


# four times the largest sine the reference shows below (measured: 4.76e-5)
QUANTISATION_SINE_BOUND = 1.9e-4


def test_what_the_quantisation_costs_on_noisy_planes():
    """40 planes of 400 points over a unit square with noise 0.002 along the normal, r = 0.12: the sine of the angle between the
    reference's normal and the eigenvector of an unquantised binary64 covariance of the same neighbours"""
    rng = np.random.default_rng(11)
    worst = 0.0
    r2, _, _ = CR.constants(0.12)
    for _ in range(40):
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        u = np.cross(nrm, [1, 0, 0])
        u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        ab = rng.uniform(-0.5, 0.5, size=(400, 2))
        noise = rng.normal(size=400) * 0.002
        P = (ab[:, :1] * u + ab[:, 1:] * v + noise[:, None] * nrm + np.array([0.3, -0.2, 3.0])).astype(np.float32)
        w = CR.brute(P, None, 0.12, 8, orient=False)
        for i in np.nonzero(w["has_normal"])[0][:60]:
            near = CR.d2_of(P[i][None, :], P) <= r2
            near[i] = False
            D = np.concatenate([(P - P[i])[near].astype(np.float64), np.zeros((1, 3))])
            D -= D.mean(axis=0)
            _, U = np.linalg.eigh(D.T @ D)
            worst = max(worst, float(np.linalg.norm(np.cross(w["normals"][i].astype(np.float64), U[:, 0]))))
    print(f"largest sine against the unquantised PCA: {worst:.3g}")
    assert worst <= QUANTISATION_SINE_BOUND


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; the lists fixed earlier and the ABI version stay"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "sgm_hip_covariance.h")).read()
    code = re.sub(r"/\*.*?\*/", "", extra, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", code)))
    L = _lib.load()
    assert declared == sorted(_lib.COVARIANCE_EXPORTS) == NEW
    assert '#include "sgm_hip_covariance.h"' in txt and all(hasattr(L, n) for n in declared)
    assert txt.index('#include "sgm_hip_statistical.h"') < txt.index('#include "sgm_hip_covariance.h"')
    earlier = dict(EXPORTS=34, CONFIDENCE_EXPORTS=1, RIGHT_EXPORTS=1, WLS_EXPORTS=3, WLS_BATCH_EXPORTS=2, LRC_EXPORTS=3,
                   VOXEL_EXPORTS=2, MESH_EXPORTS=2, NORMALS_EXPORTS=4, RADIUS_EXPORTS=2, STATISTICAL_EXPORTS=2)
    for name, length in earlier.items():
        other = getattr(_lib, name)
        assert not set(_lib.COVARIANCE_EXPORTS) & set(other) and len(other) == length, name
    assert L.sgm_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define SGM_ABI_VERSION 4\b", txt) and "sgm_hip_covariance.h" in txt.split("typedef enum")[0]
    assert all(callable(getattr(cv.Engine, n)) for n in ("covariance_normals_host", "covariance_normals_device"))
    assert callable(cv.estimate_normals_radius) and "estimate_normals_radius" in cv.__all__
    for name in NEW:      # the prototypes and the binding agree on the number of arguments
        proto = re.search(name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(getattr(L, name).argtypes) == 13
    readme = open(os.path.join(ROOT, "README.md")).read()
    for doc in (extra, cv.estimate_normals_radius.__doc__, readme):
        assert re.search(r"NOT\s+Open3D", doc.replace("**", ""), flags=re.I)
    assert "estimate_normals_radius" in readme and "voxel_down_sample" in cv.estimate_normals_radius.__doc__
    assert "write_ply(path, centroids, colors, normals)" in cv.estimate_normals_radius.__doc__
    assert _lib.COVARIANCE_STAGES == ("cov_count", "cov_clear", "cov_insert", "cov_starts", "cov_sort", "cov_query", "cov_solve")
    assert all(('"' + n + '"') in open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_engine.hip")).read()
               for n in _lib.COVARIANCE_STAGES) and all(n in extra for n in _lib.COVARIANCE_STAGES)
    assert CR.MIN_K == cv.pointcloud.COVARIANCE_MIN_NEIGHBORS == 2 and cv.pointcloud.COVARIANCE_STATS == CR.STATS
    dbg = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_debug.h")).read()
    assert re.search(r"SGM_DBG_COV_SEPARATE_SOLVE = 1 << 27\b", dbg) and _lib.SGM_DBG_COV_SEPARATE_SOLVE == 1 << 27
    assert re.search(r"SGM_DBG_COV_SELECT_ACCUM = 1 << 28\b", dbg) and _lib.SGM_DBG_COV_SELECT_ACCUM == 1 << 28
    assert list(inspect.signature(cv.estimate_normals_radius).parameters) == [
        "points_3D", "disparity_map", "radius", "min_neighbors", "origin", "viewpoint", "orient", "confidence", "min_confidence",
        "return_curvature", "return_counts", "return_stats"]
    sig = inspect.signature(cv.estimate_normals_radius).parameters
    assert sig["min_neighbors"].default == 3 and sig["orient"].default is True and sig["viewpoint"].default == (0, 0, 0)


def test_the_c_entries_refuse_without_an_engine():
    """a null engine is refused before anything touches the GPU"""
    import ctypes as C
    L = _lib.load()
    org = (C.c_float * 3)(0, 0, 0)
    st = np.full(4, 7, np.uint64)
    for fn in (L.sgm_covariance_normals, L.sgm_covariance_normals_device):
        assert fn(None, 8, None, 4, 0.05, 3, org, org, 1, None, None, None, st.ctypes.data) == -1   # SGM_ERR_INVALID_ARG
        assert b"sgm_covariance_normals" in L.sgm_last_error() and st.tolist() == [7] * 4


@pytest.fixture()
def no_engine(monkeypatch):
    """any attempt to get an engine fails the test: the errors below are raised in front of it"""
    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(S, "get_engine", boom)
    monkeypatch.setattr(S, "Engine", boom)


def test_estimate_normals_radius_argument_errors_come_before_any_engine(no_engine):
    p3, d = np.zeros((6, 9, 3), np.float32), np.ones((6, 9), np.float32)
    lst = np.zeros((10, 3), np.float32)
    enr = cv.estimate_normals_radius
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        enr(p3, d[:, :8], 0.1)
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        enr(lst, d, 0.1)
    with pytest.raises(cv.error, match=r"\(N, 3\) list"):
        enr(p3, None, 0.1)
    with pytest.raises(cv.error, match=r"\(N, 3\) list"):
        enr(np.zeros((10, 4), np.float32), None, 0.1)
    with pytest.raises(cv.error, match="estimate_normals_radius: points_3D must be float32"):
        enr(p3.astype(np.float64), d, 0.1)
    with pytest.raises(cv.error, match="confidence must have the shape"):
        enr(p3, d, 0.1, confidence=np.zeros((6, 8), np.uint8))
    with pytest.raises(cv.error, match="needs a disparity_map"):
        enr(lst, None, 0.1, confidence=np.zeros(10, np.uint8))
    for k in (0, 1, -3, 1 << 24, 1.5, True, None, "2", 2 ** 31):
        with pytest.raises(cv.error, match="min_neighbors"):
            enr(p3, d, 0.1, k)
    for r in (0, -1.0, np.nan, np.inf, 1e-45, 1e-20, 1e20, 1e39, "x", None, (1, 2)):     # 1e-20, 1e20: the square leaves the normal range
        with pytest.raises(cv.error, match="radius"):
            enr(p3, d, r)
    for o in ((0, 0), (0, 0, np.nan), (np.inf, 0, 0), 1.0, (0, 0, 0, 0), (1e39, 0, 0)):
        with pytest.raises(cv.error, match="origin"):
            enr(p3, d, 0.1, origin=o)
        with pytest.raises(cv.error, match="viewpoint"):
            enr(p3, d, 0.1, viewpoint=o)
    for orient in (0, 1, 2, None, "yes"):
        with pytest.raises(cv.error, match="orient"):
            enr(p3, d, 0.1, orient=orient)
    # an empty list needs no engine either
    out = enr(np.zeros((0, 3), np.float32), None, 0.1, return_curvature=True, return_counts=True, return_stats=True)
    assert out[0].shape == (0, 3) and out[1].shape == out[2].shape == (0,) and out[2].dtype == np.uint32
    assert out[3] == dict(in_range=0, out_of_range=0, with_normal=0, degenerate=0)
    assert enr(np.zeros((0, 3), np.float32), None, 0.1).shape == (0, 3)
    # the functions beside it raise what they raised
    with pytest.raises(cv.error, match="remove_statistical_outlier: points_3D must be float32"):
        cv.remove_statistical_outlier(p3.astype(np.float64), None, d, 4, 1.0, 0.1)
    with pytest.raises(cv.error, match="estimate_normals: points_3D must be float32"):
        cv.estimate_normals(p3.astype(np.float64), d)


def test_the_covariance_kernels_use_no_scratch():
    """resource remarks of the build: every k_cov_query instantiation and k_cov_solve without scratch memory -- the nine sums,
    the matrix and the eigenvectors stay in registers"""
    txt = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "resource_usage.txt")).read()
    blocks = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", txt, flags=re.S)
    mine = {n: (int(v), int(s)) for n, v, s in blocks if "k_cov_query" in n or "k_cov_solve" in n}
    assert len(mine) == 4 + 1, sorted(mine)
    assert all(s == 0 for _, s in mine.values()), mine
    assert all(v <= 64 for v, _ in mine.values()), mine          # eight waves per SIMD
    isa = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_engine.s")).read()
    body = isa.split("k_cov_queryILb0ELb0E", 1)[1].split("s_endpgm", 1)[0]
    assert body.count("v_mad_i64_i32") >= 6 * 4, body.count("v_mad_i64_i32")      # the six second moments of four candidates
