"""The vertex normals without a GPU: answers of the definition (include/sgm_hip_normals.h) worked by hand and held against its two
numpy restatements in tests/normals_ref.py, the two restatements against each other, the invariants the definition promises (scale,
mirror), the condition on the generated clouds that keeps the device tests from passing on trivial input, the interface lists
(header, binding, library, ABI version), the Python argument errors, all raised before any engine exists, and the PLY round trip of
write_ply / read_ply.  What the device computes is held against normals_ref.py in tests/test_gpu_normals.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import mesh_ref as MR
import normals_ref as NR
import stereo_reconstruction_cv_amd as cv
from stereo_reconstruction_cv_amd import _lib
from stereo_reconstruction_cv_amd import stereo as S
from stereo_reconstruction_cv_amd.pointcloud import estimate_normals, read_ply, triangulate_points_with_normals, write_ply  # noqa: F401
from test_mesh_reference import frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sgm_mesh_grid_normals", "sgm_mesh_grid_normals_device", "sgm_normals_grid", "sgm_normals_grid_device"]
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def both_forms(xyz, disp, md, orient):
    a, b = NR.normal_image(xyz, disp, md, orient), NR.normal_image_loop(xyz, disp, md, orient)
    assert a.dtype == b.dtype == np.float32 and np.array_equal(bits(a), bits(b))
    return a


# ---- the definition, by hand -----------------------------------------------------------------------------------------------------
def test_each_triangle_of_the_2_x_2_frame_alone():
    """frame(): X = x, Y = y, Z = 2, so every triangle lies in the plane Z = 2 with half a unit of area and its face normal, in
    the listed order, is (0, 0, -1): a = (0,0,2), c = (0,1,2), d = (1,1,2) give e1 = (0,1,0), e2 = (1,1,0), e1 x e2 = (0,0,-1).
    One triangle alone (the corner it lacks invalid, as in test_mesh_reference): its three corners get (0, 0, -1) -- s = (0,0,-1),
    m = 1, u = s, l = 1 -- and the fourth pixel, no vertex, +0.  With orient = 1: t = -1 * 2 < 0, nothing turns; the zero X and Y
    components stay +0."""
    q = [[160, 161], [162, 163]]
    for bad, named in (((0, 1), [0, 2, 3]), ((1, 0), [0, 3, 1]), ((1, 1), [0, 2, 1]), ((0, 0), [1, 2, 3])):   # T0, T1, T2, T3
        xyz, disp = frame(q, bad=[bad])
        for orient in (0, 1):
            n = both_forms(xyz, disp, 1.0, orient).reshape(4, 3)
            want = np.zeros((4, 3), np.float32)
            want[named] = (0, 0, -1)
            assert np.array_equal(bits(n), bits(want)), (bad, orient)
    # seen from behind (Z = -2): t = (-1)(-2) > 0, orient = 1 turns all three components, the +0 ones to -0
    xyz, disp = frame(q, bad=[(0, 1)])
    xyz[..., 2] = -2
    n = both_forms(xyz, disp, 1.0, 1).reshape(4, 3)
    assert np.array_equal(bits(n[[0, 2, 3]]), bits(np.array([[-0.0, -0.0, 1.0]] * 3, np.float32))) and not n[1].any()
    assert np.array_equal(bits(n[1]), bits(np.zeros(3, np.float32)))                       # the non-vertex stays +0
    assert np.array_equal(bits(both_forms(xyz, disp, 1.0, 0).reshape(4, 3)[0]), bits(np.array([0, 0, -1], np.float32)))


def test_a_flat_3_x_3_frame_gives_exactly_0_0_minus_1_everywhere():
    """all four quads take a-d (a tie) and emit both triangles; the corners have 1 or 2 triangles, the edges 3, the centre 6: the
    sums are (0, 0, -k), m = k, u = (0, 0, -1), l = 1"""
    xyz, disp = frame(np.full((3, 3), 160))
    assert NR.incident_counts(xyz, disp, 1.0).tolist() == [[2, 3, 1], [3, 6, 3], [1, 3, 2]]
    for orient in (0, 1):
        n = both_forms(xyz, disp, 1.0, orient)
        assert np.array_equal(bits(n), bits(np.broadcast_to(np.array([0, 0, -1], np.float32), (3, 3, 3))))


def test_the_exact_plane():
    """X = x 2^-7, Y = y 2^-7, Z = 2 + x 2^-9 + y 2^-10.  T0 = (a, c, d): e1 = (0, 2^-7, 2^-10), e2 = (2^-7, 2^-7, 3 * 2^-10),
    n = (3 * 2^-17 - 2^-17, 2^-17 - 0, 0 - 2^-14) = (2^-16, 2^-17, -2^-14), and the same for T1: all exact.  A sum of k of them has
    m = k 2^-14 and u = (1/4, 1/8, -1) whatever k is, so every vertex has the bits of the 3 x 3 frame's centre."""
    xyz, disp = NR.exact_plane(3, 3)
    n3 = both_forms(xyz, disp, 1.0, 1)
    centre = n3[1, 1]
    assert np.array_equal(bits(n3), bits(np.broadcast_to(centre, (3, 3, 3))))
    assert np.array_equal(bits(centre), bits(NR.exact_plane_normal()))
    exact = np.array([0.25, 0.125, -1.0]) / np.sqrt(0.25 ** 2 + 0.125 ** 2 + 1.0)
    assert (np.abs(centre.astype(np.float64) - exact) <= np.spacing(np.abs(exact).astype(np.float32))).all()   # 1 ulp per component
    for H, W in ((24, 40), (5, 131)):
        xyz, disp = NR.exact_plane(H, W)
        a, c, d = xyz[0, 0], xyz[1, 0], xyz[1, 1]
        assert np.array_equal(np.cross((c - a).astype(np.float64), (d - a).astype(np.float64)), [2.0 ** -16, 2.0 ** -17, -2.0 ** -14])
        for orient in (0, 1):
            n = NR.normal_image(xyz, disp, 0.0, orient)
            assert np.array_equal(bits(n), bits(np.broadcast_to(centre, (H, W, 3))))
    assert np.array_equal(bits(NR.normal_image_loop(*NR.exact_plane(5, 9), 0.0, 1)), bits(np.broadcast_to(centre, (5, 9, 3))))


def test_the_order_of_the_additions_is_the_face_order():
    """a 3 x 3 frame whose centre has six triangles with face normals of very different sizes, so that another order of the eight
    additions rounds differently somewhere: the two forms agree bit for bit, and the centre's sum is the sum taken by hand in
    face order"""
    rng = np.random.default_rng(5)
    xyz, disp = frame(np.full((3, 3), 160))
    xyz = (xyz * np.float32(0.37) + rng.normal(0, 0.2, size=xyz.shape) * np.array([1, 1, 3])).astype(np.float32)
    n = both_forms(xyz, disp, 1.0, 0)
    P = xyz.reshape(9, 3)
    # all quads a-d; around pixel 4: quad 0 (a=0) names it as d: T0 (0,3,4), T1 (0,4,1); quad 1 (a=1) as c: T0 (1,4,5);
    # quad 3 (a=3) as b: T1 (3,7,4); its own quad (a=4): T0 (4,7,8), T1 (4,8,5)
    s = np.zeros(3, np.float32)
    for p, q, r in ((0, 3, 4), (0, 4, 1), (1, 4, 5), (3, 7, 4), (4, 7, 8), (4, 8, 5)):
        e1, e2 = P[q] - P[p], P[r] - P[p]
        s = s + np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], np.float32)
    u = s / np.abs(s).max()
    want = u / np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    assert want.dtype == np.float32 and np.array_equal(bits(n[1, 1]), bits(want))


# ---- the two forms, and the invariants -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [2, 3, 5, 8, 9])
def test_the_vectorised_and_the_loop_form_agree_on_the_small_shape_cases(i):
    xyz, disp, _ = MR.case_input(i)
    for orient in (0, 1):
        n = both_forms(xyz, disp, MR.SHAPE_CASES[i][2], orient)
        assert np.array_equal(bits(n), bits(NR.case_want(i, orient)["image"]))
        used = MR.case_want(i)["used"]
        assert (bits(n)[~used] == 0).all()                              # non-vertices are +0, not -0
        assert ((n != 0).any(axis=2) == used).all()                     # (no sum cancels on these clouds)
        ln = np.sqrt((n[used].astype(np.float64) ** 2).sum(axis=1))
        assert np.allclose(ln, 1.0, atol=1e-6)


def test_the_two_forms_agree_on_a_crop_of_the_layered_cloud():
    xyz, disp, _ = (a[8:32, 100:140] for a in MR.layered_cloud(48, 320, 704))
    assert xyz.shape == (24, 40, 3)
    k = NR.incident_counts(xyz, disp, 0.25)
    assert all((k == j).sum() >= 10 for j in range(0, 8))
    for orient in (0, 1):
        both_forms(xyz, disp, 0.25, orient)
    x2, d2, _ = (a[8:32, 100:140] for a in NR.mixed_orientation_cloud())
    both_forms(x2, d2, 0.25, 1)
    both_forms(xyz * F32(2.0 ** 70), disp, 0.25, 1)                                 # overflowing sums take the same branch


@pytest.mark.parametrize("i", [3, 5, 6, 7, 8, 9])
def test_scaling_the_cloud_by_a_power_of_two_changes_no_bit(i):
    xyz, disp, _ = MR.case_input(i)
    md = MR.SHAPE_CASES[i][2]
    for orient in (0, 1):
        base = NR.case_want(i, orient)["image"]
        for sc in (2.0 ** -40, 2.0 ** 40):
            assert np.array_equal(bits(NR.normal_image(xyz * F32(sc), disp, md, orient)), bits(base)), (orient, sc)


@pytest.mark.parametrize("i", [5, 6, 7])
def test_mirroring_x(i):
    """X -> -X with the pixel grid as it is mirrors the cloud and reverses its winding.  Every product of step 6 that has an X in it
    changes sign and nothing else, so a face normal (nx, ny, nz) becomes (nx, -ny, -nz) exactly: with orient = 0 that is the
    normal, the mirror image of the old one turned round, which is the sign a mirrored winding gives.  Step 9's t becomes -t
    exactly, so with orient = 1 every normal with t != 0 turns the other way and comes out as the mirror image (-nx, ny, nz) of the
    old oriented one: the orientation does not depend on the winding."""
    xyz, disp, _ = MR.case_input(i)
    md = MR.SHAPE_CASES[i][2]
    mir = xyz * np.array([-1, 1, 1], np.float32)
    n0, m0 = NR.case_want(i, 0)["image"], NR.normal_image(mir, disp, md, 0)
    assert np.array_equal(m0, n0 * np.array([1, -1, -1], np.float32))
    n1, m1 = NR.case_want(i, 1)["image"], NR.normal_image(mir, disp, md, 1)
    with np.errstate(all="ignore"):
        t = (n0[..., 0] * xyz[..., 0] + n0[..., 1] * xyz[..., 1]) + n0[..., 2] * xyz[..., 2]
    live = (n0 != 0).any(axis=2) & (t != 0)
    assert live.sum() > 0.9 * MR.case_want(i)["n_vertices"]
    assert np.array_equal(m1[live], (n1 * np.array([-1, 1, 1], np.float32))[live])
    # against the winding: the mirrored unoriented normals and the mirrored oriented ones differ exactly where the old t < 0
    assert np.array_equal((m0 != m1).any(axis=2)[live], (t < 0)[live])


# ---- the condition on the generated clouds ---------------------------------------------------------------------------------------------
def test_the_generated_clouds_exercise_the_definition():
    """Every number of incident triangles, 1 .. 8, at least 200 times on both large shape cases (measured with this reference:
    906 / 1527 / 1614 / 2575 / 2682 / 2123 / 958 / 248 at 48 x 320 and 2135 / 3222 / 3484 / 5002 / 5354 / 4233 / 1972 / 515 at
    97 x 331); at scale 2^70 a share of the sums overflows and a share does not (4489 of 12633 vertices keep a normal); on the
    mixed-orientation frame step 9 turns a good part of the normals and leaves a good part (4345 of 12633 turn)."""
    for i, want in ((6, [906, 1527, 1614, 2575, 2682, 2123, 958, 248]), (7, [2135, 3222, 3484, 5002, 5354, 4233, 1972, 515])):
        xyz, disp, _ = MR.case_input(i)
        k = NR.incident_counts(xyz, disp, MR.SHAPE_CASES[i][2])
        classes = [int((k == j).sum()) for j in range(1, 9)]
        assert min(classes) >= 200 and classes == want, classes
        assert np.array_equal(k > 0, MR.case_want(i)["used"]) and k.max() == 8
    xyz, disp, _ = MR.case_input(6)
    V = MR.case_want(6)["n_vertices"]
    big = NR.normal_image(xyz * F32(2.0 ** 70), disp, 0.25, 1)
    kept = int((big != 0).any(axis=2).sum())
    assert 0.2 < kept / V < 0.8 and (kept, V) == (4489, 12633)
    assert np.isfinite(big).all()
    x2, d2, _ = NR.mixed_orientation_cloud()
    n0, n1 = NR.normal_image(x2, d2, 0.25, 0), NR.normal_image(x2, d2, 0.25, 1)
    vert = (n0 != 0).any(axis=2)
    turned = vert & (n0 != n1).any(axis=2)
    assert vert.sum() == 12633 and turned.sum() >= vert.sum() / 4 and (vert & ~turned).sum() >= vert.sum() / 4
    assert np.array_equal(n1[turned], -n0[turned]) and int(turned.sum()) == 4345
    assert (x2[..., 2][vert] < 0).sum() > 2000 and (x2[..., 2][vert] > 0).sum() > 2000


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; the lists fixed earlier and the ABI version stay"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "sgm_hip_normals.h")).read()
    code = re.sub(r"/\*.*?\*/", "", extra, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(_lib.NORMALS_EXPORTS) == NEW
    L = _lib.load()
    assert '#include "sgm_hip_normals.h"' in txt and all(hasattr(L, n) for n in declared)
    assert txt.index('#include "sgm_hip_mesh.h"') < txt.index('#include "sgm_hip_normals.h"')
    earlier = dict(EXPORTS=34, CONFIDENCE_EXPORTS=1, RIGHT_EXPORTS=1, WLS_EXPORTS=3, WLS_BATCH_EXPORTS=2, LRC_EXPORTS=3, VOXEL_EXPORTS=2,
                   MESH_EXPORTS=2)
    for name, count in earlier.items():
        other = getattr(_lib, name)
        assert len(other) == count and not set(_lib.NORMALS_EXPORTS) & set(other), name
    assert _lib.MESH_EXPORTS == ("sgm_mesh_grid", "sgm_mesh_grid_device")
    assert L.sgm_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define SGM_ABI_VERSION 4\b", txt) and "sgm_hip_normals.h" in txt.split("typedef enum")[0]
    for n in ("normals_grid_host", "normals_grid_device", "mesh_grid_normals_host", "mesh_grid_normals_device"):
        assert callable(getattr(cv.Engine, n))
    for name in ("estimate_normals", "triangulate_points_with_normals", "write_ply", "read_ply"):
        assert callable(getattr(cv, name)) and name in cv.__all__
    # the prototypes and the binding agree on the number of arguments
    for name, nargs in (("sgm_normals_grid", 8), ("sgm_normals_grid_device", 8), ("sgm_mesh_grid_normals", 14),
                        ("sgm_mesh_grid_normals_device", 14)):
        proto = re.search(r"\b" + name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(getattr(L, name).argtypes) == nargs
    # what the documents must say: our own definition, not Open3D's
    readme = open(os.path.join(ROOT, "README.md")).read()
    for doc in (extra, cv.estimate_normals.__doc__, cv.triangulate_points_with_normals.__doc__, readme.split("estimate_normals", 1)[1]):
        assert re.search(r"NOT\s+Open3D", doc.replace("**", ""), flags=re.I)
        assert "sgm_hip_normals.h" in doc
    assert "KEEP THEIR WINDING" in extra and "not pinned" in extra
    assert list(inspect.signature(cv.estimate_normals).parameters) == [
        "points_3D", "disparity_map", "max_diff", "confidence", "min_confidence", "orient"]
    assert list(inspect.signature(cv.triangulate_points_with_normals).parameters) == [
        "points_3D", "colors", "disparity_map", "max_diff", "confidence", "min_confidence", "orient"]
    assert list(inspect.signature(cv.write_ply).parameters) == ["filename", "points", "colors", "normals", "triangles", "binary"]
    assert cv.estimate_normals.__defaults__ == (1.0, None, 0, True)


def test_the_c_entries_refuse_without_an_engine():
    """a null engine is refused before anything touches the GPU, with the outputs and the counts untouched"""
    L = _lib.load()
    nv, nf = C.c_int64(-7), C.c_int64(-8)
    out = np.full((16, 3), -77.25, np.float32)
    xyz, disp = np.ones((4, 4, 3), np.float32), np.ones((4, 4), np.float32)
    for fn in (L.sgm_normals_grid, L.sgm_normals_grid_device):
        assert fn(None, xyz.ctypes.data, disp.ctypes.data, 4, 4, 1.0, 1, out.ctypes.data) == -1          # SGM_ERR_INVALID_ARG
        assert b"sgm_normals_grid" in L.sgm_last_error()
    for fn in (L.sgm_mesh_grid_normals, L.sgm_mesh_grid_normals_device):
        assert fn(None, xyz.ctypes.data, disp.ctypes.data, None, 4, 4, 1.0, 1, out.ctypes.data, None, out.ctypes.data, out.ctypes.data,
                  C.byref(nv), C.byref(nf)) == -1
        assert b"sgm_mesh_grid_normals" in L.sgm_last_error() and (nv.value, nf.value) == (-7, -8)
    assert (out == np.float32(-77.25)).all()


@pytest.fixture()
def no_engine(monkeypatch):
    """any attempt to get an engine fails the test: the errors below are raised in front of it"""
    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(S, "get_engine", boom)
    monkeypatch.setattr(S, "Engine", boom)


def test_argument_errors_come_before_any_engine(no_engine):
    p3, d, c = np.zeros((6, 9, 3), np.float32), np.ones((6, 9), np.float32), np.zeros((6, 9, 3), np.uint8)
    calls = ((lambda pts, col, disp, *a, **k: cv.estimate_normals(pts, disp, *a, **k)), cv.triangulate_points_with_normals)
    for fn in calls:
        with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
            fn(p3, c, d[:, :8])
        with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
            fn(np.zeros((54, 3), np.float32), None, d)
        with pytest.raises(cv.error, match="needs the disparity_map"):
            fn(p3, c, None)
        with pytest.raises(cv.error, match="points_3D must be float32"):
            fn(p3.astype(np.float64), c, d)
        with pytest.raises(cv.error, match="disparity_map must be float32"):
            fn(p3, c, (d * 16).astype(np.int16))
        with pytest.raises(cv.error, match="confidence must have the shape"):
            fn(p3, c, d, confidence=np.zeros((6, 8), np.uint8))
        for md in (-1.0, np.nan, np.inf, 1e39, "x", None, True):
            with pytest.raises(cv.error, match="max_diff"):
                fn(p3, c, d, md)
        big = np.broadcast_to(np.float32(1), (8193, 8192, 3)), np.broadcast_to(np.float32(1), (8193, 8192))
        with pytest.raises(cv.error, match=r"more than 67108864"):
            fn(big[0], None, big[1])
    with pytest.raises(cv.error, match="estimate_normals: "):
        cv.estimate_normals(p3, None)
    with pytest.raises(cv.error, match="triangulate_points_with_normals: colors must be uint8"):
        cv.triangulate_points_with_normals(p3, c[:5], d)
    # no quad: no device call
    for shape in ((1, 9), (6, 1), (1, 1)):
        pts, dd = np.zeros(shape + (3,), np.float32), np.ones(shape, np.float32)
        n = cv.estimate_normals(pts, dd)
        assert n.shape == shape + (3,) and n.dtype == np.float32 and (bits(n) == 0).all()
        v, k, t, n = cv.triangulate_points_with_normals(pts, np.zeros(shape + (3,), np.uint8), dd)
        assert v.shape == n.shape == (0, 3) and v.dtype == n.dtype == np.float32 and k.shape == (0, 3) and k.dtype == np.uint8
        assert t.shape == (0, 3) and t.dtype == np.int32
        assert cv.triangulate_points_with_normals(pts, None, dd, 0, orient=False)[1] is None


# ---- the PLY export ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("mesh", [True, False])
@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("with_colors", [True, False])
def test_the_ply_round_trip(tmp_path, binary, mesh, with_normals, with_colors):
    r = NR.case_want(5, 1)
    V, F = r["n_vertices"], r["n_faces"]
    assert F > 100
    path, old = str(tmp_path / "new.ply"), str(tmp_path / "old.ply")
    col = r["colors"] if with_colors else None
    nrm = r["normals"] if with_normals else None
    tri = r["faces"] if mesh else None
    assert cv.write_ply(path, r["vertices"], col, nrm, tri, binary=binary) is True
    head = open(path, "rb").read(900).decode("latin1").split("end_header")[0].split("\n")
    want = ["ply", "format binary_little_endian 1.0" if binary else "format ascii 1.0", "comment stereo_reconstruction_cv_amd",
            f"element vertex {V}", "property double x", "property double y", "property double z"]
    want += ["property double nx", "property double ny", "property double nz"] if with_normals else []
    want += ["property uchar red", "property uchar green", "property uchar blue"] if with_colors else []
    want += [f"element face {F}", "property list uchar uint vertex_indices"] if mesh else []
    assert head == want + [""]
    if binary:
        assert os.path.getsize(path) == len("\n".join(want)) + len("\nend_header\n") + V * (24 + 24 * with_normals + 3 * with_colors) + mesh * F * 13
    p, c, n, t = cv.read_ply(path)
    assert p.dtype == np.float64 and np.array_equal(p, r["vertices"].astype(np.float64))
    assert (c is None) if not with_colors else (c.dtype == np.uint8 and np.array_equal(c, r["colors"]))
    assert (n is None) if not with_normals else (n.dtype == np.float64 and np.array_equal(n, r["normals"].astype(np.float64)))
    assert (t is None) if not mesh else (t.dtype == np.int32 and np.array_equal(t, r["faces"]))
    if not with_normals:      # the bytes of the earlier writers
        if mesh:
            cv.write_triangle_mesh(old, r["vertices"], r["faces"], col, binary=binary)
        else:
            cv.write_point_cloud(old, r["vertices"], col, binary=binary)
        assert open(path, "rb").read() == open(old, "rb").read()


def test_write_ply_refuses_what_does_not_fit(tmp_path):
    path = str(tmp_path / "bad.ply")
    v = np.zeros((4, 3), np.float32)
    with pytest.raises(cv.error, match="normals and points differ"):
        cv.write_ply(path, v, normals=np.zeros((3, 3), np.float32))
    with pytest.raises(cv.error, match="colors and points differ"):
        cv.write_ply(path, v, colors=np.zeros((3, 3), np.uint8))
    with pytest.raises(cv.error, match="outside the 4 vertices"):
        cv.write_ply(path, v, triangles=np.array([[0, 1, 4]]))
    with pytest.raises(cv.error, match=r"integer \(F, 3\)"):
        cv.write_ply(path, v, triangles=np.zeros((2, 3), np.float32))
    assert not os.path.exists(path)
    # an (H, W, 3) image goes out as its H * W rows, non-finite values as they are; an empty mesh is two empty elements
    img = np.arange(24, dtype=np.float32).reshape(2, 4, 3)
    img[0, 1, 2] = np.nan
    assert cv.write_ply(path, img, normals=img[::-1])
    p, c, n, t = cv.read_ply(path)
    assert np.array_equal(p, img.reshape(-1, 3).astype(np.float64), equal_nan=True) and np.array_equal(n, img[::-1].reshape(-1, 3), equal_nan=True)
    assert c is None and t is None
    assert cv.write_ply(path, np.zeros((0, 3)), None, np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    p, c, n, t = cv.read_ply(path)
    assert p.shape == n.shape == (0, 3) and t.shape == (0, 3) and c is None
