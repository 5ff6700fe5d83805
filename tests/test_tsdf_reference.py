"""The signed distance volume without a GPU: hand-worked answers of the definition (include/sgm_hip_tsdf.h) held against its numpy
restatement tests/tsdf_ref.py -- one voxel and one pixel through every branch of the integration, one crossing on each axis --, the
two forms of each reference against each other on the case table, the order of the frames, the conditions on the generated scenes that
keep the GPU tests from passing on scenes that exercise nothing, the two helpers, the interface lists (header, binding, library,
stage names), the refusals of the C entries without an engine, the Python argument errors, all raised before any engine exists, the
scratch memory of the kernels, and the averaging on the noisy plane the feature was proposed with.  What the device computes is held
against tsdf_ref.py in tests/test_gpu_tsdf.py."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import tsdf_ref as TR
import stereo_reconstruction_cv_amd as cv
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd import stereo as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = sorted(["sgm_tsdf_integrate", "sgm_tsdf_integrate_device", "sgm_tsdf_extract_points", "sgm_tsdf_extract_points_device"])
F32, F64 = np.float32, np.float64
EYE = np.eye(4)
UNIT_CAM = (F32(1), F32(1), F32(0), F32(0))      # with a 1 x 1 frame: u = w = 0.5 for a voxel on the axis


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def one(Z, cz=4.5, tau=1.0, front=1, disp=1.0, max_depth=np.inf, w0=0, s0=0, X=0.0, Y=0.0, fn=TR.integrate):
    """one voxel with its centre at (0, 0, cz) under the identity, one pixel (X, Y, Z): (sum, weight, the counts)"""
    sm, wt, _ = TR.empty((1, 1, 1), False)
    sm[0], wt[0] = s0, w0
    xyz = np.array([[[X, Y, Z]]], F32)
    st = fn((1, 1, 1), F32(1), F32(tau), np.array([-0.5, -0.5, cz - 0.5], F32), sm, wt, None, xyz, None if disp is None else
            np.array([[disp]], F32), None, UNIT_CAM, front, EYE, max_depth)
    return int(sm[0]), int(wt[0]), st.tolist()


BOTH = pytest.mark.parametrize("fn", [TR.integrate, TR.integrate_loop], ids=["arrays", "loop"])


# ---- one voxel, one pixel ----------------------------------------------------------------------------------------------------------
@BOTH
def test_centre_camera_point_pixel_distance_and_quantum_by_hand(fn):
    """vs = 0.5, origin (1, 2, 3): c = (1.25, 2.25, 3.25).  M: a quarter turn about z, then (1, 0, 4): p = (-1.25, 1.25, 7.25).
    fx = fy = 8, cx = cy = 4 on an 8 x 8 frame: 8 * x + 4 is exact in binary64, so the fused value is its rounding.  The pixel's Z is
    p_z + 0.375: s = 0.375, q = rint(0.375 * 32767) = rint(12287.625) = 12288."""
    ext = np.array([[0.0, -1, 0, 1], [1, 0, 0, 0], [0, 0, 1, 4], [0, 0, 0, 1]])
    assert [float(v) for v in TR.camera_point(TR.m_of(ext), *[TR.centre(0, 0.5, o) for o in (1, 2, 3)])] == [-1.25, 1.25, 7.25]
    iz = F32(1) / F32(7.25)
    u = F32(F64(8) * F64(F32(-1.25) * iz) + 4) + F32(0.5)
    w = F32(F64(8) * F64(F32(1.25) * iz) + 4) + F32(0.5)
    px, py = int(np.floor(u)), int(np.floor(w))
    assert (px, py) == (3, 5)                      # 4.5 -+ 8 * 0.1724
    xyz = np.full((8, 8, 3), 100.0, F32)           # every other pixel: far behind the voxel -> clamped, q = 32767
    xyz[py, px] = (0.0, 0.0, 7.625)
    col = np.zeros((8, 8, 3), np.uint8)
    col[py, px] = (9, 250, 3)
    sm, wt, rgb = TR.empty((1, 1, 1))
    st = fn((1, 1, 1), F32(0.5), F32(1), np.array([1, 2, 3], F32), sm, wt, rgb, xyz, None, col, (8, 8, 4, 4), 1, ext)
    assert (sm[0], wt[0], rgb[:, 0].tolist()) == (12288, 1, [9, 250, 3]) and st.tolist() == [1, 1, 0, 0, 0, 0, 64, 0]


@BOTH
def test_a_pixel_coordinate_at_exactly_one_half_goes_up(fn):
    """fx = 1, cx = 0: p_x / p_z = 0.5 is the pixel coordinate 0.5, u = 1.0, pixel 1; -0.5 is u = 0, pixel 0; 1.5 is u = 2 = W: outside"""
    xyz = np.array([[[0, 0, 4.25], [0, 0, 4.5]]], F32)          # s = 0.25 through pixel 0, 0.5 through pixel 1
    for x, want in ((2.0, 16384), (-2.0, 8192), (6.0, None), (-2.0 - 2.0 ** -21, None)):
        sm, wt, _ = TR.empty((1, 1, 1), False)
        st = fn((1, 1, 1), F32(1), F32(1), np.array([x - 0.5, -0.5, 3.5], F32), sm, wt, None, xyz, None, None, UNIT_CAM, 1, EYE)
        if want is None:
            assert (sm[0], wt[0]) == (0, 0) and st.tolist() == [0, 0, 0, 0, 0, 1, 2, 0], x
        else:
            assert (sm[0], wt[0]) == (want, 1) and st.tolist() == [1, 1, 0, 0, 0, 0, 2, 0], x
    assert int(np.rint(F32(0.5) * TR.kappa_of(1))) == 16384 and int(np.rint(F32(0.25) * TR.kappa_of(1))) == 8192    # 16383.5 to even


@BOTH
def test_the_truncation_at_both_ends(fn):
    """s = -tau is kept (q = -32767), one ulp beyond is occluded; s = tau and everything above is clamped to 32767, not `unclamped`"""
    assert one(3.5, fn=fn) == (-32767, 1, [1, 1, 0, 0, 0, 0, 1, 0])
    below = float(np.nextafter(F32(3.5), F32(-np.inf)))
    assert F32(below) - F32(4.5) == F32(-1) - F32(2.0 ** -22)        # the difference is exact: s is one ulp of 3.5 beyond -tau
    assert one(below, fn=fn) == (0, 0, [0, 0, 0, 1, 0, 0, 1, 0])
    assert one(5.5, fn=fn) == (32767, 1, [1, 0, 0, 0, 0, 0, 1, 0])
    assert one(float(np.nextafter(F32(5.5), F32(0))), fn=fn)[2] == [1, 1, 0, 0, 0, 0, 1, 0]
    assert one(50.0, fn=fn) == (32767, 1, [1, 0, 0, 0, 0, 0, 1, 0])
    assert one(4.5, fn=fn) == (0, 1, [1, 1, 0, 0, 0, 0, 1, 0])
    # another tau: kappa is 32767.0f / tau, once
    assert one(4.5 + 0.3, tau=0.7, fn=fn)[0] == int(np.rint(F32(F32(4.8) - F32(4.5)) * (F32(32767) / F32(0.7))))


@BOTH
def test_behind_the_camera_and_on_its_plane(fn):
    """p_z = 0 and p_z of the wrong sign are outside, whatever the pixel holds; front = -1 mirrors everything"""
    assert one(4.0, cz=0.0, fn=fn)[2] == [0, 0, 0, 0, 0, 1, 1, 0]
    assert one(4.0, cz=-4.5, fn=fn)[2] == [0, 0, 0, 0, 0, 1, 1, 0]
    assert one(-4.0, cz=4.5, front=-1, fn=fn)[2] == [0, 0, 0, 0, 0, 1, 1, 0]
    assert one(-4.75, cz=-4.5, front=-1, fn=fn) == (8192, 1, [1, 1, 0, 0, 0, 0, 1, 0])      # the surface is 0.25 behind the voxel
    assert one(-4.25, cz=-4.5, front=-1, fn=fn)[0] == -8192
    assert one(4.75, cz=4.5, front=-1, fn=fn)[2] == [0, 0, 0, 0, 0, 1, 0, 0]               # ... and that pixel is not usable either


@BOTH
def test_pixels_without_a_depth(fn):
    for kw in (dict(Z=np.nan), dict(Z=np.inf), dict(Z=4.75, X=np.nan), dict(Z=4.75, Y=-np.inf), dict(Z=4.75, disp=0.0),
               dict(Z=4.75, disp=-1.0), dict(Z=4.75, disp=np.nan), dict(Z=-4.75), dict(Z=0.0)):
        assert one(fn=fn, **kw) == (0, 0, [0, 0, 1, 0, 0, 0, 0, 0]), kw
    assert one(4.75, disp=None, fn=fn)[1] == 1 and one(4.75, disp=1e-30, fn=fn)[1] == 1
    # max_depth is inclusive, and is about front * Z
    assert one(4.75, max_depth=4.75, fn=fn)[2] == [1, 1, 0, 0, 0, 0, 1, 0]
    assert one(4.75, max_depth=4.5, fn=fn)[2] == [0, 0, 1, 0, 0, 0, 0, 0]
    assert one(-4.75, cz=-4.5, front=-1, max_depth=4.75, fn=fn)[1] == 1 and one(-4.75, cz=-4.5, front=-1, max_depth=4.5, fn=fn)[1] == 0


@BOTH
def test_the_notebooks_q_looks_down_negative_z(fn):
    """synth.default_Q: Z = f / (-d) < 0.  camera_from_Q says front = -1; a voxel a quarter nearer to the camera than the surface of
    pixel (2, 3) gets s = +0.25"""
    H, W = 4, 6
    Q = synth.default_Q(W)
    cam, front = cv.camera_from_Q(Q)
    assert front == -1 and cam == (Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3])
    y, x = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    d = np.full((H, W), 0.5)
    h = np.stack([x + Q[0, 3], y + Q[1, 3], np.full_like(x, Q[2, 3]), Q[3, 2] * d], axis=2)
    xyz = (h[..., :3] / h[..., 3:]).astype(F32)
    assert (xyz[..., 2] < 0).all()
    tgt = xyz[2, 3].astype(F64)
    c = tgt * (1 - 0.25 / abs(tgt[2]))            # on the pixel's ray, 0.25 nearer along Z
    sm, wt, _ = TR.empty((1, 1, 1), False)
    st = fn((1, 1, 1), F32(0.125), F32(1), (c - 0.0625).astype(F32), sm, wt, None, xyz, d.astype(F32), None, cam, front, EYE)
    assert wt[0] == 1 and abs(sm[0] - 8192) <= 2 and st.tolist() == [1, 1, 0, 0, 0, 0, 24, 0]
    sm[:], wt[:] = 0, 0
    assert fn((1, 1, 1), F32(0.125), F32(1), (c - 0.0625).astype(F32), sm, wt, None, xyz, d.astype(F32), None, cam, 1, EYE)[5] == 1


@BOTH
def test_saturation_at_65535(fn):
    assert one(4.75, w0=65534, s0=7, fn=fn) == (8199, 65535, [1, 1, 0, 0, 0, 0, 1, 0])
    assert one(4.75, w0=65535, s0=7, fn=fn) == (7, 65535, [0, 0, 0, 0, 1, 0, 1, 0])
    assert one(3.0, w0=65535, fn=fn)[2] == [0, 0, 0, 1, 0, 0, 1, 0]          # occluded comes before saturated
    assert 65535 * 32767 < 2 ** 31 and 65535 * 255 < 2 ** 32


# ---- one crossing ----------------------------------------------------------------------------------------------------------------
EXTRACTS = pytest.mark.parametrize("ex", [TR.extract, TR.extract_loop], ids=["arrays", "loop"])


def pair(axis, sums, weights, rgbs=None, min_weight=1, ex=TR.extract):
    dims = [1, 1, 1]
    dims[axis] = 2
    rgb = None if rgbs is None else np.array(rgbs, np.uint32).T.copy()
    return ex(dims, F32(0.25), np.array([1, 2, 3], F32), np.array(sums, np.int32), np.array(weights, np.int32), rgb, min_weight)


@EXTRACTS
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_crossing_on_each_axis(ex, axis):
    """f0 = -100 / 1, f1 = 300 / 3: theta = -100 / -200 = 0.5, the colour of v; the means round half up in integers"""
    c = [1.125, 2.125, 3.125]
    p, col = pair(axis, [-100, 300], [1, 3], [(5, 0, 255), (4, 200, 1)], ex=ex)
    want = list(c)
    want[axis] = c[axis] + 0.5 * 0.25
    assert p.tolist() == [want] and col.tolist() == [[5, 0, 255]]
    p, col = pair(axis, [-100, 299], [1, 3], [(5, 0, 255), (4, 200, 1)], ex=ex)       # theta a little above 0.5: the colour of v'
    th = F32(-100) / (F32(-100) - F32(299) / F32(3))
    assert th > F32(0.5) and u32(p[0, axis]) == u32(TR.fmaf(th, F32(0.25), F32(c[axis]))) and col.tolist() == [[1, 67, 0]]   # 4/3, 200/3, 1/3
    p, col = pair(axis, [300, -100], [2, 1], [(5, 3, 1), (9, 9, 9)], ex=ex)           # 150 / (150 + 100) = 0.6 -> v'
    assert u32(p[0, axis]) == u32(TR.fmaf(F32(0.6), F32(0.25), F32(c[axis]))) and col.tolist() == [[9, 9, 9]]
    p, col = pair(axis, [200, -300], [2, 1], [(5, 3, 1), (9, 9, 9)], ex=ex)           # 100 / 400 -> v: 5/2 -> 3, 3/2 -> 2, 1/2 -> 1
    assert p[0, axis] == F32(c[axis] + 0.0625) and col.tolist() == [[3, 2, 1]]


@EXTRACTS
def test_zero_counts_as_not_negative_and_min_weight(ex):
    p, _ = pair(0, [0, -5], [1, 1], ex=ex)              # f0 = 0 against a negative neighbour: theta = 0, the point is c(v)
    assert p.tolist() == [[1.125, 2.125, 3.125]]
    assert pair(1, [0, 5], [1, 1], ex=ex)[0].shape == (0, 3) and pair(2, [0, 0], [1, 1], ex=ex)[0].shape == (0, 3)
    p, _ = pair(2, [-5, 0], [1, 1], ex=ex)              # theta = 1: the neighbour's centre
    assert p.tolist() == [[1.125, 2.125, 3.375]]
    assert pair(0, [-5, 5], [1, 3], min_weight=2, ex=ex)[0].shape == (0, 3) and pair(0, [-5, 5], [3, 1], min_weight=2, ex=ex)[0].shape == (0, 3)
    assert pair(0, [-5, 5], [2, 3], min_weight=2, ex=ex)[0].shape == (1, 3) and pair(0, [-5, 5], [0, 3], ex=ex)[0].shape == (0, 3)
    assert ex((1, 1, 1), F32(1), np.zeros(3, F32), np.array([-5], np.int32), np.array([1], np.int32), None, 1)[0].shape == (0, 3)


@EXTRACTS
def test_no_neighbour_past_the_faces_and_the_order(ex):
    """a 3 x 2 x 2 checkerboard of signs: every edge inside the volume crosses -- 2*2*2 + 3*1*2 + 3*2*1 = 20 of them, none past a face --
    and they come voxel by voxel, x before y before z"""
    dims = (3, 2, 2)
    k, j, i = np.meshgrid(np.arange(2), np.arange(2), np.arange(3), indexing="ij")
    sm = np.where((i + j + k) % 2 == 0, -7, 7).astype(np.int32).reshape(-1)
    wt = np.full(12, 2, np.int32)
    p = ex(dims, F32(1), np.zeros(3, F32), sm, wt, None, 1)[0]
    want = []
    for v in range(12):
        c = [v % 3 + 0.5, (v // 3) % 2 + 0.5, v // 6 + 0.5]
        for a in range(3):
            if (v % 3, (v // 3) % 2, v // 6)[a] + 1 < dims[a]:
                want.append([c[b] + (0.5 if b == a else 0.0) for b in range(3)])
    assert len(want) == 20 and p.tolist() == want


# ---- the two forms of each reference ----------------------------------------------------------------------------------------------
SMALL = [c for c in TR.cases() if c[0] != (40, 32, 24)]
# The 40 x 32 x 24 cases of the table are too many voxels for the loops in full: every one of them runs here on a 10 x 8 x 6 stand-in
# over the same region -- a SUBSTITUTION --, and the real volume meets the loops in test_the_loops_on_the_real_40_x_32_x_24_volume.
COARSE = [((10, 8, 6), hw, en, fr, col, dsp) for dims, hw, en, fr, col, dsp in TR.cases() if dims == (40, 32, 24)]


@pytest.mark.parametrize("case", SMALL + COARSE, ids=lambda c: "%dx%dx%d-%dx%d-e%d%+d" % (c[0] + c[1] + (c[2], c[3])))
def test_arrays_and_loops_agree(case):
    a = TR.case_input(case)
    (s1, w1, c1), st1 = TR.run_case(a)
    (s2, w2, c2), st2 = TR.run_case(a, fn=TR.integrate_loop)
    assert st1.tolist() == st2.tolist() and (s1 == s2).all() and (w1 == w2).all() and (c1 is None or (c1 == c2).all())
    assert int(st1[:6].sum() - st1[1]) == s1.size
    b = TR.case_input(case, seed=5)                          # a second frame: crossings need weights, and colours need sums
    b["ext"] = a["ext"]
    TR.run_case(b, (s1, w1, c1))
    for mw in (1, 2):
        p1, k1 = TR.extract(a["dims"], a["vs"], a["origin"], s1, w1, c1, mw)
        p2, k2 = TR.extract_loop(a["dims"], a["vs"], a["origin"], s1, w1, c1, mw)
        assert u32(p1).tolist() == u32(p2).tolist() and (k1 is None or k1.tolist() == k2.tolist())


def test_the_loops_on_the_real_40_x_32_x_24_volume():
    """the volume the GPU tests use, not its stand-in: integrate_loop on five of its slabs through the z-range form (the first, the
    last, three in the middle where the wall and the box lie) against the same slabs of the array form, after two frames; then
    extract_loop over the WHOLE volume against the array form"""
    case = ((40, 32, 24), (48, 64), 1, -1, True, True)
    frames = [TR.case_input(case, seed=s) for s in (0, 5)]
    full = TR.empty((40, 32, 24))
    for f in frames:
        TR.run_case(f, full)
    nxy = 40 * 32
    seen = 0
    for z0, z1 in ((0, 1), (8, 9), (11, 13), (23, 24)):
        pl = TR.empty((40, 32, z1 - z0))
        for f in frames:
            TR.run_case(f, pl, fn=TR.integrate_loop, z0=z0, z1=z1)
        assert (pl[0] == full[0][z0 * nxy:z1 * nxy]).all() and (pl[1] == full[1][z0 * nxy:z1 * nxy]).all(), (z0, z1)
        assert (pl[2] == full[2][:, z0 * nxy:z1 * nxy]).all(), (z0, z1)
        seen += int((pl[1] > 0).sum())
    assert seen > 1000
    a = frames[0]
    for mw in (1, 2):
        p1, c1 = TR.extract(a["dims"], a["vs"], a["origin"], *full, mw)
        p2, c2 = TR.extract_loop(a["dims"], a["vs"], a["origin"], *full, mw)
        assert p1.shape[0] > 500 and u32(p1).tolist() == u32(p2).tolist() and c1.tolist() == c2.tolist(), mw


def test_slabs_are_the_volume():
    """the z-range form: each slab on its own slice of the planes gives the whole volume's bytes and counts"""
    a = TR.case_input(((40, 32, 24), (48, 64), 1, -1, True, True))
    (s, w, c), st = TR.run_case(a)
    nxy = 40 * 32
    tot = np.zeros(8, np.uint64)
    for z0, z1 in ((0, 1), (1, 13), (13, 23), (23, 24)):
        pl = TR.empty((40, 32, z1 - z0))
        t = TR.run_case(a, pl, z0=z0, z1=z1)[1]
        assert (pl[0] == s[z0 * nxy:z1 * nxy]).all() and (pl[1] == w[z0 * nxy:z1 * nxy]).all() and (pl[2] == c[:, z0 * nxy:z1 * nxy]).all()
        tot[:6] += t[:6]
        assert t[6] == st[6]
    assert tot[:6].tolist() == st[:6].tolist()


def three_frames(color=True):
    out = []
    for k, en in enumerate((0, 1, 2)):
        a = TR.case_input(((40, 32, 24), (48, 64), en, 1, color, True), seed=k)
        a["vs"], a["origin"] = TR.volume_for((40, 32, 24), np.eye(4))          # one volume, three poses
        out.append(a)
    return out


def test_three_frames_in_all_six_orders_give_the_same_bytes():
    frames = three_frames()
    first = None
    for order in itertools.permutations(range(3)):
        pl = TR.empty((40, 32, 24))
        for k in order:
            TR.run_case(frames[k], pl)
        got = [p.tobytes() for p in pl]
        first = first or got
        assert got == first, order
    assert pl[1].max() == 3 and (pl[1] == 1).any() and (pl[1] == 2).any()


def test_the_generated_scenes_exercise_what_they_claim():
    """each 48 x 64 scene in the 40 x 32 x 24 volume holds updated, clamped, occluded, no-depth and outside voxels, and its
    extraction at least one crossing per axis; the wave-edge volumes hold updates on both sides of column 63"""
    for case in [c for c in TR.cases() if c[0] == (40, 32, 24) and c[1] == (48, 64)]:
        a = TR.case_input(case)
        (s, w, c), st = TR.run_case(a)
        upd, uncl, nod, occ, sat, outs = (int(v) for v in st[:6])
        assert uncl > 100 and upd - uncl > 100 and nod > 100 and occ > 100 and outs > 100 and sat == 0, (case, st)
        axes = TR.extract(a["dims"], a["vs"], a["origin"], s, w, c, 1, with_axis=True)[2]
        assert all((axes == k).sum() >= 10 for k in range(3)), (case, np.bincount(axes))
        assert (s < 0).any() and (s > 0).any()
    edge = [TR.run_case(TR.case_input(c))[0][1].reshape(2, 3, 65) for c in TR.cases() if c[0] == (65, 3, 2) and c[1] == (48, 64)]
    assert any(w[..., 64].any() and w[..., 63].any() and w[..., :63].any() for w in edge) and all(w.any() for w in edge)


# ---- the helpers -----------------------------------------------------------------------------------------------------------------
def test_camera_from_q_and_invert_rigid():
    Q = synth.default_Q(480)
    assert cv.camera_from_Q(Q) == ((Q[2, 3], Q[2, 3], 1909.9754 * 480 / 3840, 1057.74529 * 480 / 3840), -1)
    P = Q.copy()
    P[3, 2] = 2.0
    assert cv.camera_from_Q(P)[1] == 1
    for bad in (np.eye(3), 2 * Q, np.full((4, 4), np.nan), "abcd", np.diag([1.0, 1, 0, 0])):
        with pytest.raises(cv.error, match="camera_from_Q"):
            cv.camera_from_Q(bad)
    for T in TR.EXTRINSICS:
        inv = cv.invert_rigid(T)
        assert inv.dtype == np.float64 and np.abs(inv - np.linalg.inv(T)).max() < 1e-15 * 4 and inv[3].tolist() == [0, 0, 0, 1]
        assert np.abs(inv @ T - np.eye(4)).max() < 1e-15 * 4
    for bad in (None, np.eye(3), np.ones((4, 4)), np.full((4, 4), np.inf)):
        with pytest.raises(cv.error, match="invert_rigid"):
            cv.invert_rigid(bad)


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; the lists fixed earlier and the ABI version stay"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "sgm_hip_tsdf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", extra, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", code)))
    L = _lib.load()
    assert declared == sorted(_lib.TSDF_EXPORTS) == NEW
    assert '#include "sgm_hip_tsdf.h"' in txt and all(hasattr(L, n) for n in declared)
    assert txt.index('#include "sgm_hip_icp.h"') < txt.index('#include "sgm_hip_tsdf.h"')
    earlier = dict(EXPORTS=34, CONFIDENCE_EXPORTS=1, RIGHT_EXPORTS=1, WLS_EXPORTS=3, WLS_BATCH_EXPORTS=2, LRC_EXPORTS=3,
                   VOXEL_EXPORTS=2, MESH_EXPORTS=2, NORMALS_EXPORTS=4, RADIUS_EXPORTS=2, STATISTICAL_EXPORTS=2, COVARIANCE_EXPORTS=2,
                   DBSCAN_EXPORTS=2, PLANE_EXPORTS=4, ICP_EXPORTS=7)
    for name, length in earlier.items():
        other = getattr(_lib, name)
        assert not set(_lib.TSDF_EXPORTS) & set(other) and len(other) == length, name
    assert L.sgm_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define SGM_ABI_VERSION 4\b", txt) and "sgm_hip_tsdf.h" in txt.split("typedef enum")[0]
    counts = dict(sgm_tsdf_integrate=18, sgm_tsdf_integrate_device=18, sgm_tsdf_extract_points=12, sgm_tsdf_extract_points_device=12)
    for name in NEW:      # the prototypes and the binding agree on the number of arguments
        proto = re.search(r"\b" + name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(getattr(L, name).argtypes) == counts[name], name
    assert _lib.TSDF_STAGES == ("tsdf_integrate", "tsdf_count", "tsdf_scan", "tsdf_emit")
    engine = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "sgm_engine.hip")).read()
    assert all(('"' + n + '"') in engine for n in _lib.TSDF_STAGES) and all(n in extra for n in _lib.TSDF_STAGES)
    assert "&e->tsdf_sum, &e->tsdf_w, &e->tsdf_rgb, &e->tsdf_cnt, &e->tsdf_off" in engine      # sgm_trim gives them back
    readme = open(os.path.join(ROOT, "README.md")).read()
    for doc in (extra, cv.TSDFVolume.__doc__, readme.split("TSDFVolume", 1)[1]):
        assert re.search(r"NOT\s+Open3D", doc.replace("**", ""), flags=re.I)
    for gap in ("hashed or sparse", "scaled with depth", "weights other than 1", "normals from the gradient", "marching-cubes", "ray casting",
                "batch of frames"):
        assert gap in re.sub(r"\s+\*?\s*", " ", extra), gap
    assert "in any order gives the same bytes" in re.sub(r"\s+\*?\s*", " ", extra) and "Saturation is where that ends" in extra
    names = {"TSDFVolume", "camera_from_Q", "invert_rigid"}
    assert all(callable(getattr(cv, n)) for n in names) and names <= set(cv.__all__) and all(n in readme for n in names)
    assert all(callable(getattr(cv.Engine, n)) for n in ("tsdf_integrate_host", "tsdf_integrate_device", "tsdf_extract_host", "tsdf_extract_device"))
    assert cv.pointcloud.TSDF_STATS == TR.STATS and cv.pointcloud.TSDF_MAX_WEIGHT == TR.MAX_WEIGHT and cv.pointcloud.TSDF_MAX_DIM == TR.MAX_DIM
    chain = re.sub(r"\s+", " ", cv.TSDFVolume.__doc__)
    assert "registration_icp(frame k, frame 0)" in chain and "extract_point_cloud -> estimate_normals_radius -> write_ply" in chain
    assert "sgm_hip_tsdf.h" in open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "Makefile")).read()
    assert "sgm_tsdf_integrate" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    kernels = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "kernels_tsdf.h")).read()
    assert "__builtin_fmaf" in kernels and "atomicAdd(&stats" in kernels and "__builtin_rintf" in kernels
    body = kernels[kernels.index("void k_tsdf_integrate("):kernels.index("void k_tsdf_usable(")]
    plain, counts = body.split("if constexpr (STATS)")
    assert "__shared__" not in plain and "atomicAdd" not in plain          # the volume: no LDS, no atomics
    assert counts.count("atomicAdd(&stats") == 1 and counts.count("atomicAdd(&wg") == 1      # the counts: one global atomic instruction per workgroup


def vol_args(color=True, n=(2, 2, 2)):
    V = n[0] * n[1] * n[2]
    return dict(dims=np.array(n, np.int32), org=np.zeros(3, F32), sm=np.full(V, 7, np.int32), wt=np.full(V, 7, np.int32),
                rgb=np.full((3, V), 7, np.uint32) if color else None, xyz=np.ones((2, 3, 3), F32), col=np.ones((2, 3, 3), np.uint8),
                cam=np.array([1, 1, 1, 1], F32), T=np.eye(4).reshape(16).copy(), st=np.full(8, 7, np.uint64), pts=np.full((5, 3), 7, F32),
                pc=np.full((5, 3), 7, np.uint8))


def untouched(a):
    return all((a[k] == 7).all() for k in ("sm", "wt", "rgb", "st", "pts", "pc") if a[k] is not None)


def at(x):
    return None if x is None else x.ctypes.data


def test_the_c_entries_refuse_without_an_engine_and_bad_arguments():
    """a null engine, and every argument the header names, is refused before anything touches the GPU, with nothing touched.  The
    argument checks come after the engine's, so they are made with a pointer that is never followed: the refusals come first"""
    L = _lib.load()
    a = vol_args()
    tot = C.c_int64(-9)

    def integ(fn, e=None, **kw):
        b = dict(a, vs=0.5, tau=1.0, H=2, W=3, front=1, md=np.inf)
        b.update(kw)
        return fn(e, at(b["dims"]), b["vs"], b["tau"], at(b["org"]), at(b["sm"]), at(b["wt"]), at(b["rgb"]), at(b["xyz"]), None, at(b["col"]),
                  b["H"], b["W"], at(b["cam"]), b["front"], at(b["T"]), b["md"], at(b["st"]))

    def extr(fn, e=None, **kw):
        b = dict(a, vs=0.5, mw=1, cap=5)
        b.update(kw)
        return fn(e, at(b["dims"]), b["vs"], at(b["org"]), at(b["sm"]), at(b["wt"]), at(b["rgb"]), b["mw"], b["cap"], at(b["pts"]), at(b["pc"]),
                  C.byref(tot))

    def named(name):      # the error text begins with the entry's own name: the device entries say _device
        return L.sgm_last_error().startswith(name.encode() + b":")
    for name in ("sgm_tsdf_integrate", "sgm_tsdf_integrate_device"):
        assert integ(getattr(L, name)) == -1 and named(name) and untouched(a)
    for name in ("sgm_tsdf_extract_points", "sgm_tsdf_extract_points_device"):
        assert extr(getattr(L, name)) == -1 and named(name) and untouched(a) and tot.value == -9
    # the other refusals need an engine pointer that is not null; none of them follows it
    fake = C.c_void_p(C.addressof(C.create_string_buffer(1 << 16)))
    nanT, rowT = a["T"].copy(), a["T"].copy()
    nanT[3], rowT[15] = np.nan, 2.0
    bad_int = [dict(sm=None), dict(wt=None), dict(xyz=None), dict(dims=None), dict(org=None), dict(cam=None), dict(T=None), dict(col=None),
               dict(rgb=None), dict(front=0), dict(front=2), dict(cam=np.array([1, np.inf, 1, 1], F32)), dict(vs=0.0), dict(vs=-1.0),
               dict(vs=np.nan), dict(tau=0.0), dict(tau=np.inf), dict(tau=-1.0), dict(tau=1e-38), dict(org=np.array([0, np.nan, 0], F32)),
               dict(T=nanT), dict(T=rowT), dict(md=0.0), dict(md=-1.0), dict(md=np.nan), dict(H=0), dict(W=-1)]
    for name in ("sgm_tsdf_integrate", "sgm_tsdf_integrate_device"):
        fn = getattr(L, name)
        for kw in bad_int:
            assert integ(fn, fake, **kw) == -1 and named(name) and untouched(a), kw
        for kw in (dict(dims=np.array([0, 1, 1], np.int32)), dict(dims=np.array([1, 4097, 1], np.int32)),
                   dict(dims=np.array([1024, 1024, 1025], np.int32)), dict(H=1 << 14, W=(1 << 13) + 1)):
            assert integ(fn, fake, **kw) == -4 and named(name) and untouched(a), kw      # SGM_ERR_UNSUPPORTED
    assert 32767.0 / 1e-38 > 3.5e38                     # ... the kappa that is not finite in binary32
    for name in ("sgm_tsdf_extract_points", "sgm_tsdf_extract_points_device"):
        fn = getattr(L, name)
        for kw in (dict(sm=None), dict(wt=None), dict(dims=None), dict(org=None), dict(mw=0), dict(mw=-3), dict(cap=-1), dict(rgb=None),
                   dict(pts=None), dict(vs=0.0), dict(org=np.array([np.inf, 0, 0], F32))):
            assert extr(fn, fake, **kw) == -1 and named(name) and untouched(a) and tot.value == -9, kw
        assert extr(fn, fake, dims=np.array([4096, 4096, 65], np.int32)) == -4 and tot.value == -9


@pytest.fixture()
def no_engine(monkeypatch):
    """any attempt to get an engine fails the test: the errors below are raised in front of it"""
    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(S, "get_engine", boom)
    monkeypatch.setattr(S, "Engine", boom)


def test_argument_errors_come_before_any_engine(no_engine):
    V = cv.TSDFVolume
    for bad in (0, -1.0, np.nan, np.inf, "x", None, True, 1e-50):
        with pytest.raises(cv.error, match="voxel_size"):
            V(bad, 1.0, (2, 2, 2), device=False)
        with pytest.raises(cv.error, match="sdf_trunc"):
            V(0.5, bad, (2, 2, 2), device=False)
    with pytest.raises(cv.error, match="32767 / sdf_trunc"):
        V(0.5, 1e-38, (2, 2, 2), device=False)
    for bad in ((2, 2), (0, 2, 2), (2, 4097, 2), (2.0, 2, 2), 5, None, (True, 2, 2), "abc"):
        with pytest.raises(cv.error, match="dims"):
            V(0.5, 1.0, bad, device=False)
    with pytest.raises(cv.error, match="2\\^30"):
        V(0.5, 1.0, (1024, 1024, 1025), device=False)
    for bad in ((0, 0), (0, np.nan, 0), "ab", None):
        with pytest.raises(cv.error, match="origin"):
            V(0.5, 1.0, (2, 2, 2), origin=bad, device=False)
    vol = V(0.5, 1.0, (4, 3, 2), origin=(1, 2, 3), device=False)
    assert vol.device is None and vol.sum.shape == (2, 3, 4) and vol.sum.dtype == np.int32 and vol.weight.dtype == np.int32
    assert vol.rgb_sum.shape == (3, 2, 3, 4) and vol.rgb_sum.dtype == np.uint32 and V(0.5, 1.0, (4, 3, 2), color=False, device=False).rgb_sum is None
    vol.sum[:] = 5
    vol.rgb_sum[:] = 6
    vol.reset()
    assert not vol.sum.any() and not vol.rgb_sum.any() and not vol.weight.any()
    xyz, d, col = np.ones((6, 9, 3), F32), np.ones((6, 9), F32), np.ones((6, 9, 3), np.uint8)
    cam = (10.0, 10.0, 4.0, 2.5)
    ig = vol.integrate
    with pytest.raises(cv.error, match="points_3D must be float32"):
        ig(xyz.astype(F64), col, d, cam)
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        ig(xyz, col, d[:, :8], cam)
    with pytest.raises(cv.error, match=r"\(H, W, 3\)"):
        ig(xyz.reshape(-1, 3), col, None, cam)
    with pytest.raises(cv.error, match="disparity_map must be float32"):
        ig(xyz, col, d.astype(F64), cam)
    with pytest.raises(cv.error, match="confidence map needs a disparity_map"):
        ig(xyz, col, None, cam, confidence=d)
    with pytest.raises(cv.error, match="the volume has colour"):
        ig(xyz, None, d, cam)
    for bad in (col.astype(np.int32), col[:5]):
        with pytest.raises(cv.error, match="colors must be uint8"):
            ig(xyz, bad, d, cam)
    for bad in ((1, 2, 3), (1, 2, 3, np.nan), "abcd", None, np.eye(3)):
        with pytest.raises(cv.error, match="intrinsic"):
            ig(xyz, col, d, bad)
    for bad in (np.eye(3), np.full((4, 4), np.nan), np.diag([1.0, 1, 1, 2]), "abcd"):
        with pytest.raises(cv.error, match="extrinsic"):
            ig(xyz, col, d, cam, extrinsic=bad)
    for bad in (0, 2, -2, 1.5, True, "x"):
        with pytest.raises(cv.error, match="front"):
            ig(xyz, col, d, cam, front=bad)
    for bad in (0, -1.0, np.nan, "x", True):
        with pytest.raises(cv.error, match="max_depth"):
            ig(xyz, col, d, cam, max_depth=bad)
    for bad in (0, -1, 1.5, True, None, "2"):
        with pytest.raises(cv.error, match="min_weight"):
            vol.extract_point_cloud(bad)


def test_the_tsdf_kernels_use_no_scratch():
    """resource remarks of the build: every kernel of kernels_tsdf.h without scratch memory, the integration without LDS"""
    txt = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "resource_usage.txt")).read()
    blocks = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", txt, flags=re.S)
    mine = {n: (int(v), int(s), int(l)) for n, v, s, l in blocks if "k_tsdf_" in n}
    assert len(mine) == 6, sorted(mine)       # integrate without and with the counts, usable, count, scan, emit
    for name, (vgprs, scratch, lds) in mine.items():
        assert scratch == 0 and vgprs <= 128, (name, vgprs, scratch)
    plain = [v for n, v in mine.items() if "k_tsdf_integrateILb0E" in n]
    assert len(plain) == 1 and plain[0][2] == 0 and plain[0][0] <= 32, plain      # the kernel every frame runs: no LDS


# ---- what it is for ----------------------------------------------------------------------------------------------------------------
def test_eight_noisy_frames_are_better_than_one():
    """The scene the feature was proposed with (a fronto-parallel plane at Z = 10, f = 60, disparity noise 0.15 -- a depth noise of
    about 0.25 --, 0.25 voxels, trunc 1.0), on the reference alone: the rms Z error of the crossings is 0.2289 after one frame and
    0.0991 after eight.  Eight independent frames can at best divide it by sqrt(8) = 2.8; the interpolation between
    0.25 voxels and the clamped tails keep some of it.  Asserted: better, and by at least a third -- half of what was measured
    (a factor 2.3), so that another seed of the same scene passes too."""
    r1, n1 = TR.quality_rms(1)
    r8, n8 = TR.quality_rms(8)
    print("rms Z error: one frame %.4f (%d crossings), eight frames %.4f (%d crossings)" % (r1, n1, r8, n8))
    assert n1 > 1000 and n8 > 1000
    assert r8 < r1 and r8 < r1 / 1.5
    assert 0.15 < r1 < 0.3           # one frame is about its depth noise
