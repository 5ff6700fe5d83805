"""The grid triangulation without a GPU: hand-worked answers of the definition (include/sgm_hip_mesh.h) held against its numpy
restatement tests/mesh_ref.py, index sanity and the closed form of the ramp, the condition on the generated clouds that keeps the
device tests from passing on trivial input, the interface lists (header, binding, library, ABI version), the Python argument errors,
all of which are raised before any engine exists, and the PLY round trip.  What the device computes is held against mesh_ref.py in
tests/test_gpu_mesh.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import mesh_ref as MR
import stereo_reconstruction_cv_amd as cv
from stereo_reconstruction_cv_amd import _lib
from stereo_reconstruction_cv_amd import stereo as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sgm_mesh_grid", "sgm_mesh_grid_device"]
NAN, INF = float("nan"), float("inf")
# the four candidate triangles of the one quad of a 2 x 2 frame, in pixel numbers a = 0, b = 1, c = 2, d = 3
T0, T1, T2, T3 = [0, 2, 3], [0, 3, 1], [0, 2, 1], [1, 2, 3]


def frame(sixteenths, bad=()):
    """a frame whose disparities are given in sixteenths of a pixel (exact in binary32); X grows with x, Y with y, Z = 2.
    bad: pixels (y, x) whose Y is NaN"""
    disp = np.asarray(sixteenths, np.float32) / np.float32(16)
    H, W = disp.shape
    y, x = np.mgrid[0:H, 0:W]
    xyz = np.stack([x, y, np.full((H, W), 2)], axis=2).astype(np.float32)
    for p in bad:
        xyz[p][1] = np.nan
    return xyz, disp


def tris(sixteenths, max_diff, bad=()):
    """the emitted triangles in PIXEL numbers, as lists"""
    xyz, disp = frame(sixteenths, bad)
    r = MR.mesh_grid(xyz, disp, None, max_diff)
    assert r["faces"].dtype == np.int32 and r["vertices"].dtype == np.float32
    assert np.array_equal(r["vertices"], xyz.reshape(-1, 3)[r["pixels"]])
    return r["pixels"][r["faces"]].tolist()


# ---- the definition, by hand -----------------------------------------------------------------------------------------------------
def test_the_smooth_quad_gives_t0_then_t1():
    """all four disparities equal: the diagonal differences tie at 0, a-d is taken, both triangles are connected"""
    assert tris([[160, 160], [160, 160]], 1.0) == [T0, T1]
    xyz, disp = frame([[160, 160], [160, 160]])
    r = MR.mesh_grid(xyz, disp, np.arange(12, dtype=np.uint8).reshape(2, 2, 3), 1.0)
    assert (r["n_vertices"], r["n_faces"]) == (4, 2) and r["colors"].tolist() == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]]
    # the winding: with X along x, Y along y and Z away from the camera every normal (q - p) x (r - p) points at the camera, -Z
    for t in (T0, T1, T2, T3):
        p, q, s = xyz.reshape(-1, 3)[t].astype(np.float64)
        assert np.cross(q - p, s - p)[2] < 0


def test_each_corner_invalid_in_turn_leaves_the_one_triangle_of_the_other_three():
    """a invalid: no a-d, so b-c, whose T3 = (b, c, d) lacks a.  b invalid: a and d valid and b, c not both: a-d, T0 = (a, c, d).
    c invalid: a-d, T1 = (a, d, b).  d invalid: b-c, T2 = (a, c, b)."""
    q = [[160, 161], [162, 163]]
    for bad, want in (((0, 0), T3), ((0, 1), T0), ((1, 0), T1), ((1, 1), T2)):
        assert tris(q, 1.0, bad=[bad]) == [want], bad
        d0 = np.array(q)
        d0[bad] = 0                                   # ... and the same by a disparity of 0
        assert tris(d0, 1.0) == [want], bad
    for two in (((0, 0), (1, 1)), ((0, 1), (1, 0)), ((0, 0), (0, 1))):
        assert tris(q, 100.0, bad=two) == []          # two valid corners make no triangle


def test_a_tie_of_the_diagonal_differences_takes_a_d_and_a_smaller_b_c_difference_takes_b_c():
    """a = 10, d = 10.25, b = 10.5, c = 10.25: |a - d| = |b - c| = 4 sixteenths -- a tie: a-d.
    c one sixteenth nearer to b: |b - c| = 3 < 4: b-c.  a one sixteenth nearer to d instead: 3 < 4: a-d."""
    assert tris([[160, 168], [164, 164]], 1.0) == [T0, T1]
    assert tris([[160, 168], [165, 164]], 1.0) == [T2, T3]
    assert tris([[161, 168], [164, 164]], 1.0) == [T0, T1]


def test_an_edge_exactly_at_max_diff_connects_and_one_sixteenth_above_does_not():
    """max_diff = 0.5 = 8 sixteenths.  a = 160, b = 168, c = 160, d = 164: a-d (4 < 8).  T1 = (a, d, b) has a-b at exactly 8:
    connected.  With b = 169 the edge a-b is 9 sixteenths: T1 goes, T0 = (a, c, d) stays."""
    assert tris([[160, 168], [160, 164]], 0.5) == [T0, T1]
    assert tris([[160, 169], [160, 164]], 0.5) == [T0]


def test_max_diff_zero_connects_only_equal_disparities():
    assert tris([[160, 160], [160, 160]], 0.0) == [T0, T1]
    assert tris([[160, 161], [160, 160]], 0.0) == [T0]            # a-d ties b-c?  |a - d| = 0 < 1: a-d; T1 needs a-b: gone
    assert tris([[160, 160], [161, 160]], 0.0) == [T1]
    assert tris([[160, 161], [161, 160]], 0.0) == []


def test_nan_in_y_alone_and_nonpositive_disparities_make_a_pixel_invalid():
    """a 3 x 3 frame, the centre invalid: each of the four quads has three valid corners and emits its one triangle; the centre
    is no vertex"""
    for kind in ("nan", "zero", "negative", "nan disparity"):
        xyz, disp = frame(np.full((3, 3), 160))
        if kind == "nan":
            xyz[1, 1, 1] = np.nan
        else:
            disp[1, 1] = dict(zero=0.0, negative=-3.0)[kind] if kind != "nan disparity" else np.nan
        r = MR.mesh_grid(xyz, disp, None, 1.0)
        # quad (0,0) lacks d: T2 = (0, 3, 1); (0,1) lacks c: T1 = (1, 5, 2); (1,0) lacks b: T0 = (3, 6, 7); (1,1) lacks a: T3 = (5, 7, 8)
        assert r["pixels"][r["faces"]].tolist() == [[0, 3, 1], [1, 5, 2], [3, 6, 7], [5, 7, 8]], kind
        assert r["pixels"].tolist() == [0, 1, 2, 3, 5, 6, 7, 8] and not r["used"][1, 1]
        assert r["faces"].tolist() == [[0, 3, 1], [1, 4, 2], [3, 5, 6], [4, 6, 7]]     # numbered past the hole


def test_an_infinite_disparity_gives_no_triangle_with_it():
    """+inf > 0, so the pixel is VALID (the quad does not fall back to three corners), but inf - x is inf and inf - inf is NaN:
    no edge to it connects.  b = inf: |b - c| = inf, a-d is taken, T0 = (a, c, d) stays and T1 names b: gone.
    a = inf: |a - d| = inf > |b - c|: b-c, T3 = (b, c, d) stays.  a = d = inf: |a - d| is NaN, which is not <= anything: b-c,
    and both its triangles have an edge to a or d."""
    i = np.float32(np.inf) * 16
    assert tris([[160, i], [160, 160]], 100.0) == [T0]
    assert tris([[i, 160], [160, 160]], 100.0) == [T3]
    assert tris([[i, 160], [160, i]], 100.0) == []
    assert tris([[i, i], [i, i]], 100.0) == []
    assert MR.valid_mask(*frame([[i, 160], [160, 160]])).all()


def test_a_chosen_diagonal_whose_edge_fails_emits_nothing_even_where_the_other_would():
    """The diagonal is chosen from the two differences alone, never from what would be emitted.
    a = 160, b = 180, c = d = 170, max_diff = 1 (16 sixteenths): |a - d| = |b - c| = 10, a tie: a-d.  T0 = (a, c, d) connects;
    T1 = (a, d, b) has a-b = 20 and goes.  T3 = (b, c, d) of the OTHER diagonal has b-c = 10, c-d = 0, b-d = 10 and would connect:
    it is not emitted, the quad keeps one triangle.  Mirrored: b-c chosen, T3 lost to b-d, T0 of the other diagonal connected.
    Then the chosen diagonal's own edge failing: a = 160, d = 192, c = 176 and b invalid takes a-d (b and c are not both valid),
    a-d = 32 exceeds max_diff = 1.5 (24 sixteenths), and nothing is emitted although a-c and c-d (16 each) connect."""
    assert tris([[160, 180], [170, 170]], 1.0) == [T0]
    # a = 160, b = 177, c = 176, d = 162: |b - c| = 1 < |a - d| = 2: b-c.  T2 = (a, c, b) has a-b = 17 and goes, T3 stays
    # (1, 14, 15); T0 = (a, c, d) of the other diagonal (16, 14, 2) would connect
    assert tris([[160, 177], [176, 162]], 1.0) == [T3]
    assert tris([[160, 160], [176, 192]], 1.5, bad=[(0, 1)]) == []
    assert tris([[160, 160], [176, 184]], 1.5, bad=[(0, 1)]) == [T0]        # (a-d = 24: exactly at max_diff)
    assert tris([[160, 176], [208, 192]], 1.5) == []                # all valid, a tie at 32: a-d, which fails, and so does b-c


# ---- index sanity on the generated clouds, and the ramp in closed form ---------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(MR.SHAPE_CASES)))
def test_index_sanity_on_the_generated_clouds(i):
    H, W, md = MR.SHAPE_CASES[i]
    r = MR.case_want(i)
    V, F = r["n_vertices"], r["n_faces"]
    assert r["vertices"].shape == (V, 3) and r["colors"].shape == (V, 3) and r["faces"].shape == (F, 3)
    if H < 2 or W < 2:
        assert (V, F) == (0, 0)
        return
    f = r["faces"]
    assert f.size == 0 or (f.min() >= 0 and f.max() < V)                              # every index lies in [0, V)
    assert np.array_equal(np.unique(f), np.arange(V))                                 # every vertex is used
    assert (np.diff(r["pixels"]) > 0).all()                                           # ascending pixel order
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()  # no repeated index
    assert r["valid"].reshape(-1)[r["pixels"]].all()                                   # only valid pixels are vertices
    assert F == int(r["first"].sum()) + int(r["second"].sum()) <= 2 * (H - 1) * (W - 1)
    xyz, disp, col = MR.case_input(i)
    assert np.array_equal(r["vertices"].view(np.uint32), xyz.reshape(-1, 3)[r["pixels"]].view(np.uint32))
    assert np.array_equal(r["colors"], col.reshape(-1, 3)[r["pixels"]])
    assert MR.case_want(i, with_colors=False)["colors"] is None
    # the faces of a quad come first triangle first, quads row-major: the smallest pixel of a face (its quad's a, or b for T3)
    # never runs backwards by more than one pixel
    head = r["pixels"][f].min(axis=1)
    assert (np.diff(head) >= -1).all()


@pytest.mark.parametrize("H,W", [(2, 2), (2, 65), (3, 257), (48, 320)])
def test_the_ramp_in_closed_form(H, W):
    xyz, disp, col = MR.ramp_cloud(H, W)
    r = MR.mesh_grid(xyz, disp, col, 0.0)
    assert r["n_vertices"] == H * W and r["n_faces"] == 2 * (H - 1) * (W - 1)
    assert np.array_equal(r["faces"], MR.ramp_faces(H, W)) and np.array_equal(r["pixels"], np.arange(H * W))
    assert np.array_equal(r["vertices"], xyz.reshape(-1, 3)) and np.array_equal(r["colors"], col.reshape(-1, 3))
    k = 2 * ((H - 2) * (W - 1) + (W - 2))                        # the last quad's two faces by the formula
    a = (H - 2) * W + W - 2
    assert r["faces"][k].tolist() == [a, a + W, a + W + 1] and r["faces"][k + 1].tolist() == [a, a + W + 1, a + 1]


def cloud_stats(H, W, seed, md):
    xyz, disp, col = MR.layered_cloud(H, W, seed)
    r = MR.mesh_grid(xyz, disp, col, md)
    v = r["valid"]
    corners = va, vb, vc, vd = v[:-1, :-1], v[:-1, 1:], v[1:, :-1], v[1:, 1:]
    nvalid = va.astype(int) + vb + vc + vd
    emitted = r["first"].astype(int) + r["second"]
    four, three = nvalid == 4, nvalid == 3
    return dict(ratio=r["n_faces"] / (2 * (H - 1) * (W - 1)), ad=int((four & ~r["bc"]).sum()), bc=int((four & r["bc"]).sum()),
                single=[int((three & ~m & (emitted == 1)).sum()) for m in corners], four_one=int((four & (emitted == 1)).sum()),
                unused=int((v & ~r["used"]).sum()), three_all=bool((emitted[three] == 1).all()), few=int(emitted[nvalid < 3].sum()))


def test_the_generated_clouds_exercise_the_definition():
    """The mix must not quietly degenerate: about half of the possible triangles, both diagonals, every kind of single triangle,
    four-valid quads that lose one of their two, and valid pixels that no triangle uses.  Measured with this reference at
    48 x 320, seed 704, max_diff 0.25: 0.57 / 4618 / 4518 / 855, 871, 885, 862 / 1796 / 1069; at 97 x 331, seed 705: 9693 / 9637 /
    1793, 1817, 1762, 1805 / 3425 / 2494.  The bounds are asserted there and, doubled, at the larger frame; the two shapes of
    SHAPE_CASES (seeds 706 and 707) are held to the same."""
    assert [c[:2] for c in MR.SHAPE_CASES[:8]] == [(1, 1), (1, 64), (2, 2), (2, 63), (2, 65), (3, 257), (48, 320), (97, 331)]
    assert [c[:2] for c in MR.SHAPE_CASES[8:]] == [(3, 1028), (2, 1025)]          # one past the block of 1024 pixels, in both load forms
    assert MR.SHAPE_CASES[6][2] == MR.SHAPE_CASES[7][2] == 0.25
    for (H, W, seed), k in (((48, 320, 704), 1), ((48, 320, 706), 1), ((97, 331, 705), 2), ((97, 331, 707), 2)):
        s = cloud_stats(H, W, seed, 0.25)
        assert 0.4 < s["ratio"] < 0.75, s
        assert s["ad"] > 1000 * k and s["bc"] > 1000 * k, s
        assert min(s["single"]) > 500 * k and s["four_one"] > 500 * k and s["unused"] > 500 * k, s
        assert s["few"] == 0 and not s["three_all"], s
    s = cloud_stats(48, 320, 704, 0.25)
    assert (round(s["ratio"], 2), s["ad"], s["bc"], s["single"], s["four_one"], s["unused"]) == (0.57, 4618, 4518, [855, 871, 885, 862], 1796, 1069)
    s = cloud_stats(97, 331, 705, 0.25)
    assert (s["ad"], s["bc"], s["single"], s["four_one"], s["unused"]) == (9693, 9637, [1793, 1817, 1762, 1805], 3425, 2494)
    # at max_diff = 100 every edge between valid pixels connects: every three-valid quad emits, no four-valid quad loses one, and
    # only pixels without a complete neighbourhood stay unused
    for (H, W, seed), unused in (((48, 320, 704), 8), ((97, 331, 705), 13)):
        s = cloud_stats(H, W, seed, 100.0)
        assert s["unused"] == unused and s["three_all"] and s["four_one"] == 0, s
    # the small shapes of the list are not all empty
    assert sum(MR.case_want(i)["n_faces"] for i in (2, 3, 4, 5)) > 100 and MR.case_want(2)["n_faces"] >= 1
    assert MR.case_want(8)["n_faces"] > 100 and MR.case_want(9)["n_faces"] > 100


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; the lists fixed earlier and the ABI version stay"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "sgm_hip_mesh.h")).read()
    code = re.sub(r"/\*.*?\*/", "", extra, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(_lib.MESH_EXPORTS) == NEW
    L = _lib.load()
    assert '#include "sgm_hip_mesh.h"' in txt and all(hasattr(L, n) for n in declared)
    for other in (_lib.EXPORTS, _lib.CONFIDENCE_EXPORTS, _lib.RIGHT_EXPORTS, _lib.WLS_EXPORTS, _lib.WLS_BATCH_EXPORTS, _lib.LRC_EXPORTS,
                  _lib.VOXEL_EXPORTS):
        assert not set(_lib.MESH_EXPORTS) & set(other)
    assert L.sgm_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define SGM_ABI_VERSION 4\b", txt) and "sgm_hip_mesh.h" in txt.split("typedef enum")[0]
    assert all(callable(getattr(cv.Engine, n)) for n in ("mesh_grid_host", "mesh_grid_device"))
    for name in ("triangulate_points", "write_triangle_mesh", "read_triangle_mesh"):
        assert callable(getattr(cv, name)) and name in cv.__all__
    # the prototypes and the binding agree on the number of arguments
    for name in NEW:
        proto = re.search(name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(getattr(L, name).argtypes) == 12
    # what the documents must say: our own definition, not Open3D's
    for doc in (extra, cv.triangulate_points.__doc__, open(os.path.join(ROOT, "README.md")).read().split("triangulate_points", 1)[1]):
        assert re.search(r"NOT\s+Open3D", doc.replace("**", ""), flags=re.I)
    assert "sgm_hip_mesh.h" in cv.triangulate_points.__doc__
    assert MR.MAX_PIXELS == cv.pointcloud.MESH_MAX_PIXELS == 1 << 26 >= 4096 * 2160
    assert list(inspect.signature(cv.triangulate_points).parameters) == [
        "points_3D", "colors", "disparity_map", "max_diff", "confidence", "min_confidence"]
    assert list(inspect.signature(cv.write_triangle_mesh).parameters) == ["filename", "vertices", "triangles", "colors", "binary"]
    # the earlier writers keep their signatures
    assert list(inspect.signature(cv.write_point_cloud).parameters) == ["filename", "points", "colors", "binary"]


def test_the_c_entries_refuse_without_an_engine():
    """a null engine is refused before anything touches the GPU, with the counts untouched"""
    L = _lib.load()
    nv, nf = C.c_int64(-7), C.c_int64(-8)
    for fn in (L.sgm_mesh_grid, L.sgm_mesh_grid_device):
        assert fn(None, 8, 8, None, 4, 4, 1.0, 16, None, 16, C.byref(nv), C.byref(nf)) == -1      # SGM_ERR_INVALID_ARG
        assert b"sgm_mesh_grid" in L.sgm_last_error() and (nv.value, nf.value) == (-7, -8)


@pytest.fixture()
def no_engine(monkeypatch):
    """any attempt to get an engine fails the test: the errors below are raised in front of it"""
    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(S, "get_engine", boom)
    monkeypatch.setattr(S, "Engine", boom)


def test_triangulate_points_argument_errors_come_before_any_engine(no_engine):
    p3, d, c = np.zeros((6, 9, 3), np.float32), np.ones((6, 9), np.float32), np.zeros((6, 9, 3), np.uint8)
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        cv.triangulate_points(p3, c, d[:, :8])
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        cv.triangulate_points(np.zeros((54, 3), np.float32), None, d)
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        cv.triangulate_points(np.zeros((6, 9, 4), np.float32), None, d)
    with pytest.raises(cv.error, match="needs the disparity_map"):
        cv.triangulate_points(p3, c, None)
    with pytest.raises(cv.error, match="points_3D must be float32"):
        cv.triangulate_points(p3.astype(np.float64), c, d)
    with pytest.raises(cv.error, match="disparity_map must be float32"):
        cv.triangulate_points(p3, c, (d * 16).astype(np.int16))
    with pytest.raises(cv.error, match="colors must be uint8"):
        cv.triangulate_points(p3, c[:5], d)
    with pytest.raises(cv.error, match="colors must be uint8"):
        cv.triangulate_points(p3, c.astype(np.float32), d)
    with pytest.raises(cv.error, match="confidence must have the shape"):
        cv.triangulate_points(p3, c, d, confidence=np.zeros((6, 8), np.uint8))
    for md in (-1.0, -1e-30, np.nan, np.inf, -np.inf, 1e39, "x", None, (1, 2), True):
        with pytest.raises(cv.error, match="max_diff"):
            cv.triangulate_points(p3, c, d, md)
    # frames over the limit (the arrays are views of one value: nothing of that size is allocated)
    big = np.broadcast_to(np.float32(1), (8193, 8192, 3)), np.broadcast_to(np.float32(1), (8193, 8192))
    with pytest.raises(cv.error, match=r"more than 67108864"):
        cv.triangulate_points(big[0], None, big[1])
    # no quad: empty arrays without a device call
    for shape in ((1, 9), (6, 1), (1, 1)):
        v, k, t = cv.triangulate_points(np.zeros(shape + (3,), np.float32), np.zeros(shape + (3,), np.uint8), np.ones(shape, np.float32))
        assert v.shape == (0, 3) and v.dtype == np.float32 and k.shape == (0, 3) and k.dtype == np.uint8
        assert t.shape == (0, 3) and t.dtype == np.int32
        assert cv.triangulate_points(np.zeros(shape + (3,), np.float32), None, np.ones(shape, np.float32), 0)[1] is None


# ---- the PLY export ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("with_colors", [True, False])
def test_the_ply_round_trip(tmp_path, binary, with_colors):
    r = MR.case_want(5)
    assert r["n_faces"] > 100
    path = str(tmp_path / "mesh.ply")
    col = r["colors"] if with_colors else None
    assert cv.write_triangle_mesh(path, r["vertices"], r["faces"], col, binary=binary) is True
    head = open(path, "rb").read(600).decode("latin1").split("end_header")[0].split("\n")
    want = ["ply", "format binary_little_endian 1.0" if binary else "format ascii 1.0", "comment stereo_reconstruction_cv_amd",
            f"element vertex {r['n_vertices']}", "property double x", "property double y", "property double z"]
    want += ["property uchar red", "property uchar green", "property uchar blue"] if with_colors else []
    want += [f"element face {r['n_faces']}", "property list uchar uint vertex_indices", ""]
    assert head == want
    if binary:
        assert os.path.getsize(path) == len("\n".join(want)) + len("end_header\n") + r["n_vertices"] * (24 + 3 * with_colors) + r["n_faces"] * 13
    v, c, t = cv.read_triangle_mesh(path)
    assert v.dtype == np.float64 and np.array_equal(v, r["vertices"].astype(np.float64))
    assert (c is None) if not with_colors else (c.dtype == np.uint8 and np.array_equal(c, r["colors"]))
    assert t.dtype == np.int32 and np.array_equal(t, r["faces"])


def test_the_ply_writer_refuses_what_is_no_mesh(tmp_path):
    path = str(tmp_path / "bad.ply")
    v = np.zeros((4, 3), np.float32)
    for t in ([[0, 1, 4]], [[0, -1, 2]], [[0, 1, 2], [3, 2, 2 ** 31]]):
        with pytest.raises(cv.error, match="outside the 4 vertices"):
            cv.write_triangle_mesh(path, v, np.array(t, np.int64))
    with pytest.raises(cv.error, match=r"integer \(F, 3\)"):
        cv.write_triangle_mesh(path, v, np.zeros((2, 4), np.int32))
    with pytest.raises(cv.error, match=r"integer \(F, 3\)"):
        cv.write_triangle_mesh(path, v, np.zeros((2, 3), np.float32))
    with pytest.raises(cv.error, match="colors must be uint8"):
        cv.write_triangle_mesh(path, v, np.array([[0, 1, 2]], np.int32), np.zeros((3, 3), np.uint8))
    assert not os.path.exists(path)
    # an empty mesh is a file with two empty elements
    assert cv.write_triangle_mesh(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v, c, t = cv.read_triangle_mesh(path)
    assert v.shape == (0, 3) and c is None and t.shape == (0, 3)
