"""The signed distance volume on the GPU (include/sgm_hip_tsdf.h) against its numpy restatement tests/tsdf_ref.py, bit for bit: the
planes, all eight counts, the extracted points, colours and totals, through the host and the device entries, with and without
colours, disparities and counts; the hand cases of tests/test_tsdf_reference.py on the device; frames that miss the volume;
capacities; saturation; the order of the frames; repeated calls; an engine with a history and poisoned buffers; the stage record and
the refusals; the calls beside it unchanged; the Python class; two frames from the pipeline; a volume whose planes pass 2^31 bytes;
and the cases once more with every buffer guarded."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import icp_ref as IR
import parity_util as U
import tsdf_ref as TR
import voxel_ref as VR
import stereo_reconstruction_cv_amd as sgm
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = dict(numDisparities=16)
F32 = np.float32
EYE = np.eye(4)
MARK = 7


@pytest.fixture(scope="module")
def eng():
    return Engine(P16)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    """a numpy array as a HIP tensor of the same bytes (uint32 planes as int32), None as None"""
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def integrate(e, entry, a, planes, stats=True, max_depth=np.inf):
    """one frame (a dict of tsdf_ref.case_input) into the numpy planes, in place, through the host or the device entry: the counts"""
    s, w, rgb = planes
    if entry == "host":
        return e.tsdf_integrate_host(a["dims"], a["vs"], a["tau"], a["origin"], s, w, rgb, a["xyz"], a["disp"], a["colors"], a["cam"], a["front"],
                                     a["ext"], max_depth, stats)
    import torch
    ts, tw, tr, tx, td, tc = (dev(x) for x in (s, w, rgb, a["xyz"], a["disp"], a["colors"]))
    H, W = a["xyz"].shape[:2]
    torch.cuda.synchronize()
    st = e.tsdf_integrate_device(a["dims"], a["vs"], a["tau"], a["origin"], ptr(ts), ptr(tw), ptr(tr), ptr(tx), ptr(td), ptr(tc), H, W, a["cam"],
                                 a["front"], a["ext"], max_depth, stats)
    e.synchronize()
    s[:], w[:] = ts.cpu().numpy(), tw.cpu().numpy()
    if rgb is not None:
        rgb[:] = tr.cpu().numpy().view(np.uint32)
    return st


def extract(e, entry, a, planes, min_weight=1, cap=None, colors=True):
    """(total, points (cap, 3), colours (cap, 3) or None): the rows past the count keep MARK.  cap None: count first, as the class does"""
    s, w, rgb = planes
    colors = colors and rgb is not None
    if entry == "host":
        if cap is None:
            cap = e.tsdf_extract_host(a["dims"], a["vs"], a["origin"], s, w, rgb, min_weight)
        pts, col = np.full((cap, 3), MARK, F32), (np.full((cap, 3), MARK, np.uint8) if colors else None)
        total = e.tsdf_extract_host(a["dims"], a["vs"], a["origin"], s, w, rgb, min_weight, pts if cap else None, col if cap else None)
        return total, pts, col
    import torch
    ts, tw, tr = dev(s), dev(w), dev(rgb)
    torch.cuda.synchronize()
    if cap is None:
        cap = e.tsdf_extract_device(a["dims"], a["vs"], a["origin"], ptr(ts), ptr(tw), ptr(tr), min_weight)
    tp = torch.full((cap, 3), float(MARK), dtype=torch.float32, device="cuda")
    tc = torch.full((cap, 3), MARK, dtype=torch.uint8, device="cuda") if colors else None
    torch.cuda.synchronize()
    total = e.tsdf_extract_device(a["dims"], a["vs"], a["origin"], ptr(ts), ptr(tw), ptr(tr), min_weight, cap, ptr(tp) if cap else None,
                                  ptr(tc) if cap else None)
    assert np.array_equal(ts.cpu().numpy(), s) and np.array_equal(tw.cpu().numpy(), w)         # the extraction never touches the planes
    return total, tp.cpu().numpy(), None if tc is None else tc.cpu().numpy()


_cache = {}


def want_case(i, frames=2):
    """the reference of case i after one and after `frames` frames, computed once and shared (read-only):
    [(planes, counts of the last frame, points, colours)] per number of frames"""
    if i not in _cache:
        case = TR.cases()[i]
        pl = TR.empty(case[0], case[4])
        out = []
        for k in range(frames):
            a = TR.case_input(case, seed=5 * k)
            st = TR.run_case(a, pl)[1]
            p, c = TR.extract(a["dims"], a["vs"], a["origin"], *pl, 1)
            out.append((tuple(None if x is None else x.copy() for x in pl), st, p, c))
        _cache[i] = out
    return _cache[i]


def same_planes(got, want, what=""):
    for g, w, name in zip(got, want, ("sum", "weight", "rgb_sum")):
        assert (g is None) == (w is None) and (g is None or np.array_equal(g, w)), (what, name, None if g is None else int((g != w).sum()))


def same_cloud(got, wp, wc, what=""):
    total, pts, col = got
    n = wp.shape[0]
    k = min(n, pts.shape[0])
    assert total == n, (what, total, n)
    assert np.array_equal(u32(pts[:k]), u32(wp[:k])) and (pts[k:] == MARK).all(), (what, int((u32(pts[:k]) != u32(wp[:k])).sum()))
    if col is not None:
        assert np.array_equal(col[:k], wc[:k]) and (col[k:] == MARK).all(), what


# ---- 1. the case table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ("host", "device"))
@pytest.mark.parametrize("i", range(len(TR.cases())), ids=lambda i: "%dx%dx%d-%dx%d-e%d%+d" % (TR.cases()[i][0] + TR.cases()[i][1] + TR.cases()[i][2:4]))
def test_cases_through_both_entries(eng, i, entry):
    """every volume with every frame, two frames each: the planes and the eight counts after each frame, the extraction after each"""
    case = TR.cases()[i]
    pl = TR.empty(case[0], case[4])
    for k, (wpl, wst, wp, wc) in enumerate(want_case(i)):
        a = TR.case_input(case, seed=5 * k)
        st = integrate(eng, entry, a, pl)
        assert st.tolist() == wst.tolist(), (case, k, st, wst)
        same_planes(pl, wpl, (case, k))
        same_cloud(extract(eng, entry, a, pl), wp, wc, (case, k))
    # without the counts: the same bytes, and no colours from a colour volume
    pl2 = TR.empty(case[0], case[4])
    for k in range(2):
        assert integrate(eng, entry, TR.case_input(case, seed=5 * k), pl2, stats=False) is None
    same_planes(pl2, wpl, (case, "no stats"))
    same_cloud(extract(eng, entry, a, pl2, colors=False), wp, None, (case, "no colours"))
    same_cloud(extract(eng, entry, a, pl2, min_weight=2), *TR.extract(a["dims"], a["vs"], a["origin"], *wpl, 2), (case, "min_weight 2"))


# ---- 2. the hand cases, on the device ------------------------------------------------------------------------------------------
def one(e, entry, Z, cz=4.5, tau=1.0, front=1, disp=1.0, max_depth=np.inf, w0=0, s0=0, X=0.0, Y=0.0):
    a = dict(dims=(1, 1, 1), vs=F32(1), tau=F32(tau), origin=np.array([-0.5, -0.5, cz - 0.5], F32), xyz=np.array([[[X, Y, Z]]], F32),
             disp=None if disp is None else np.array([[disp]], F32), colors=None, cam=(1, 1, 0, 0), front=front, ext=EYE)
    pl = TR.empty((1, 1, 1), False)
    pl[0][0], pl[1][0] = s0, w0
    st = integrate(e, entry, a, pl, max_depth=max_depth)
    return int(pl[0][0]), int(pl[1][0]), st.tolist()


@pytest.mark.parametrize("entry", ("host", "device"))
def test_one_voxel_and_one_pixel_by_hand(eng, entry):
    o = lambda *a, **k: one(eng, entry, *a, **k)
    assert o(3.5) == (-32767, 1, [1, 1, 0, 0, 0, 0, 1, 0])                                   # s = -tau is kept
    assert o(float(np.nextafter(F32(3.5), F32(-np.inf)))) == (0, 0, [0, 0, 0, 1, 0, 0, 1, 0])  # one ulp beyond: occluded
    assert o(5.5) == (32767, 1, [1, 0, 0, 0, 0, 0, 1, 0]) and o(50.0) == (32767, 1, [1, 0, 0, 0, 0, 0, 1, 0])
    assert o(float(np.nextafter(F32(5.5), F32(0))))[2] == [1, 1, 0, 0, 0, 0, 1, 0] and o(4.5) == (0, 1, [1, 1, 0, 0, 0, 0, 1, 0])
    assert o(4.8, tau=0.7)[0] == int(np.rint(F32(F32(4.8) - F32(4.5)) * (F32(32767) / F32(0.7))))
    assert o(4.0, cz=0.0)[2] == [0, 0, 0, 0, 0, 1, 1, 0] and o(4.0, cz=-4.5)[2] == [0, 0, 0, 0, 0, 1, 1, 0]      # p_z = 0, p_z behind
    assert o(-4.75, cz=-4.5, front=-1) == (8192, 1, [1, 1, 0, 0, 0, 0, 1, 0]) and o(-4.25, cz=-4.5, front=-1)[0] == -8192
    assert o(4.75, cz=4.5, front=-1)[2] == [0, 0, 0, 0, 0, 1, 0, 0]
    for kw in (dict(Z=np.nan), dict(Z=np.inf), dict(Z=4.75, X=np.nan), dict(Z=4.75, Y=-np.inf), dict(Z=4.75, disp=0.0), dict(Z=4.75, disp=-1.0),
               dict(Z=4.75, disp=np.nan), dict(Z=-4.75), dict(Z=0.0)):
        assert o(**kw) == (0, 0, [0, 0, 1, 0, 0, 0, 0, 0]), kw
    assert o(4.75, disp=None)[1] == 1
    assert o(4.75, max_depth=4.75)[2] == [1, 1, 0, 0, 0, 0, 1, 0] and o(4.75, max_depth=4.5)[2] == [0, 0, 1, 0, 0, 0, 0, 0]
    assert o(4.75, w0=65534, s0=7) == (8199, 65535, [1, 1, 0, 0, 0, 0, 1, 0])               # the last frame a voxel takes
    assert o(4.75, w0=65535, s0=7) == (7, 65535, [0, 0, 0, 0, 1, 0, 1, 0]) and o(3.0, w0=65535)[2] == [0, 0, 0, 1, 0, 0, 1, 0]
    # a pixel coordinate at exactly one half goes up; u = W is outside
    xyz = np.array([[[0, 0, 4.25], [0, 0, 4.5]]], F32)
    for x, want in ((2.0, 16384), (-2.0, 8192), (6.0, None), (-2.0 - 2.0 ** -21, None)):
        a = dict(dims=(1, 1, 1), vs=F32(1), tau=F32(1), origin=np.array([x - 0.5, -0.5, 3.5], F32), xyz=xyz, disp=None, colors=None,
                 cam=(1, 1, 0, 0), front=1, ext=EYE)
        pl = TR.empty((1, 1, 1), False)
        st = integrate(eng, entry, a, pl)
        assert (int(pl[0][0]), int(pl[1][0]), st.tolist()) == ((0, 0, [0, 0, 0, 0, 0, 1, 2, 0]) if want is None else (want, 1, [1, 1, 0, 0, 0, 0, 2, 0])), x
    # the quarter turn of the CPU file: centre, camera point, pixel (5, 3), s = 0.375, q = 12288, and the colour of that pixel
    ext = np.array([[0.0, -1, 0, 1], [1, 0, 0, 0], [0, 0, 1, 4], [0, 0, 0, 1]])
    xyz = np.full((8, 8, 3), 100.0, F32)
    xyz[5, 3] = (0.0, 0.0, 7.625)
    col = np.zeros((8, 8, 3), np.uint8)
    col[5, 3] = (9, 250, 3)
    a = dict(dims=(1, 1, 1), vs=F32(0.5), tau=F32(1), origin=np.array([1, 2, 3], F32), xyz=xyz, disp=None, colors=col, cam=(8, 8, 4, 4), front=1, ext=ext)
    pl = TR.empty((1, 1, 1))
    assert integrate(eng, entry, a, pl).tolist() == [1, 1, 0, 0, 0, 0, 64, 0] and (pl[0][0], pl[1][0], pl[2][:, 0].tolist()) == (12288, 1, [9, 250, 3])


@pytest.mark.parametrize("entry", ("host", "device"))
def test_one_crossing_by_hand_on_each_axis(eng, entry):
    for axis in range(3):
        dims = [1, 1, 1]
        dims[axis] = 2
        a = dict(dims=dims, vs=F32(0.25), origin=np.array([1, 2, 3], F32))
        c = [1.125, 2.125, 3.125]

        def ex(sums, weights, rgbs, mw=1):
            pl = (np.array(sums, np.int32), np.array(weights, np.int32), np.array(rgbs, np.uint32).T.copy())
            total, p, col = extract(eng, entry, a, pl, mw, cap=2)
            assert (p[total:] == MARK).all() and (col[total:] == MARK).all()
            return total, p[:total], col[:total]
        n, p, col = ex([-100, 300], [1, 3], [(5, 0, 255), (4, 200, 1)])                    # theta = 0.5: the colour of v
        want = list(c)
        want[axis] += 0.125
        assert n == 1 and p.tolist() == [want] and col.tolist() == [[5, 0, 255]]
        n, p, col = ex([-100, 299], [1, 3], [(5, 0, 255), (4, 200, 1)])                    # a little above: the colour of v'
        th = F32(-100) / (F32(-100) - F32(299) / F32(3))
        assert n == 1 and u32(p[0, axis]) == u32(TR.fmaf(th, F32(0.25), F32(c[axis]))) and col.tolist() == [[1, 67, 0]]
        n, p, col = ex([200, -300], [2, 1], [(5, 3, 1), (9, 9, 9)])                        # the means round half up
        assert n == 1 and p[0, axis] == F32(c[axis] + 0.0625) and col.tolist() == [[3, 2, 1]]
        n, p, col = ex([0, -5], [1, 1], [(1, 1, 1), (2, 2, 2)])                            # f0 = 0 against a negative neighbour
        assert n == 1 and p.tolist() == [c]
        assert ex([0, 5], [1, 1], [(1, 1, 1), (2, 2, 2)])[0] == 0 and ex([-5, 5], [1, 3], [(1, 1, 1), (2, 2, 2)], 2)[0] == 0
        assert ex([-5, 5], [2, 3], [(1, 1, 1), (2, 2, 2)], 2)[0] == 1
    # no neighbour past the faces, and the order: the 3 x 2 x 2 checkerboard of the CPU file
    k, j, i = np.meshgrid(np.arange(2), np.arange(2), np.arange(3), indexing="ij")
    pl = (np.where((i + j + k) % 2 == 0, -7, 7).astype(np.int32).reshape(-1), np.full(12, 2, np.int32), None)
    a = dict(dims=(3, 2, 2), vs=F32(1), origin=np.zeros(3, F32))
    same_cloud(extract(eng, entry, a, pl, cap=25), *TR.extract_loop((3, 2, 2), F32(1), np.zeros(3, F32), *pl), "checkerboard")
    assert extract(eng, entry, a, pl, cap=0)[0] == 20


# ---- 3. nothing to do ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ("host", "device"))
def test_frames_that_miss_the_volume_and_frames_without_a_pixel(eng, entry):
    """a volume behind the camera, one beside the frustum, one beyond max_depth's reach, an all-NaN and an all-nonpositive frame:
    nothing is written -- the planes keep the poison they were given"""
    case = ((40, 32, 24), (48, 64), 1, 1, True, True)
    a = TR.case_input(case)
    rng = np.random.default_rng(3)
    V = 40 * 32 * 24

    def poisoned():
        return (rng.integers(-9999, 9999, V).astype(np.int32), rng.integers(0, 65536, V).astype(np.int32),
                rng.integers(0, 1 << 24, (3, V)).astype(np.uint32))
    for what, kw, counts in (("behind", dict(front=-1, xyz=-a["xyz"]), (5,)), ("beside", dict(origin=a["origin"] + F32(500.0)), (5,)),
                             ("all nan", dict(xyz=np.full_like(a["xyz"], np.nan)), (2, 5)), ("no disparity", dict(disp=np.zeros_like(a["disp"])), (2, 5)),
                             ("too far", dict(), (2, 5))):
        b = dict(a, **kw)          # ("behind": the scene mirrored; the volume stays where it was, behind the mirrored camera's back)
        pl = poisoned()
        keep = tuple(x.copy() for x in pl)
        st = integrate(eng, entry, b, pl, max_depth=1.0 if what == "too far" else np.inf)
        same_planes(pl, keep, what)
        ref = tuple(x.copy() for x in keep)
        wst = TR.run_case(b, ref, max_depth=1.0 if what == "too far" else np.inf)[1]
        assert st.tolist() == wst.tolist() and st[0] == 0 and st[4] == 0 and sum(int(st[c]) for c in counts) == V, (what, st)
        same_planes(ref, keep, what)
    # an empty volume has no crossings, and neither has one that nobody saw twice
    empty = TR.empty((40, 32, 24))
    assert extract(eng, entry, a, empty, cap=4)[0] == 0 and extract(eng, entry, a, want_case(14, 2)[0][0], min_weight=2, cap=4)[0] == 0


# ---- 4. capacity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ("host", "device"))
def test_capacity_below_equal_and_above_the_total(eng, entry):
    i = 15
    a = TR.case_input(TR.cases()[i])
    wpl, _, wp, wc = want_case(i)[1]
    n = wp.shape[0]
    assert n > 2000
    for cap in (0, 1, 255, n - 1, n, n + 1, n + 1000):
        got = extract(eng, entry, a, wpl, cap=cap)
        assert got[1].shape[0] == cap
        same_cloud(got, wp, wc, cap)
    same_cloud(extract(eng, entry, a, wpl, cap=n, colors=False), wp, None, "points only")


# ---- 5. saturation, order, repetition --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ("host", "device"))
def test_a_volume_one_frame_from_full_and_a_full_one(eng, entry):
    a = TR.case_input(TR.cases()[15])
    V = 40 * 32 * 24
    for w0 in (65534, 65535):
        pl = (np.full(V, 1000, np.int32), np.full(V, w0, np.int32), np.full((3, V), 12345, np.uint32))
        ref = tuple(x.copy() for x in pl)
        wst = TR.run_case(a, ref)[1]
        st = integrate(eng, entry, a, pl)
        assert st.tolist() == wst.tolist() and (st[0], st[4])[w0 - 65534] > 10000 and (st[4], st[0])[w0 - 65534] == 0
        same_planes(pl, ref, w0)
        assert pl[1].max() == 65535
    # mixed: every third voxel full
    pl = TR.empty((40, 32, 24))
    pl[1][::3] = 65535
    ref = tuple(x.copy() for x in pl)
    wst = TR.run_case(a, ref)[1]
    assert integrate(eng, entry, a, pl).tolist() == wst.tolist() and wst[0] > 1000 and wst[4] > 1000
    same_planes(pl, ref, "mixed")


def three_frames():
    out = []
    for k, en in enumerate((0, 1, 2)):
        a = TR.case_input(((40, 32, 24), (48, 64), en, 1, True, True), seed=k)
        a["vs"], a["origin"] = TR.volume_for((40, 32, 24), np.eye(4))
        out.append(a)
    return out


@pytest.mark.parametrize("entry", ("host", "device"))
def test_three_frames_in_six_orders(eng, entry):
    frames = three_frames()
    want = TR.empty((40, 32, 24))
    for f in frames:
        TR.run_case(f, want)
    wp, wc = TR.extract((40, 32, 24), frames[0]["vs"], frames[0]["origin"], *want, 1)
    for order in itertools.permutations(range(3)):
        pl = TR.empty((40, 32, 24))
        for k in order:
            integrate(eng, entry, frames[k], pl, stats=(k == 1))
        same_planes(pl, want, order)
    same_cloud(extract(eng, entry, frames[0], pl), wp, wc, "three frames")
    assert want[1].max() == 3 and wp.shape[0] > 1000


def test_five_calls_give_the_same_bytes(eng):
    i = 16
    a = TR.case_input(TR.cases()[i])
    wpl, wst, wp, wc = want_case(i)[0]
    for entry in ("host", "device"):
        runs = []
        for _ in range(5):
            pl = TR.empty(a["dims"], a["colors"] is not None)
            st = integrate(eng, entry, a, pl)
            got = extract(eng, entry, a, pl)
            runs.append(b"".join(np.ascontiguousarray(x).tobytes() for x in list(pl) + [st, got[1], got[2]] if x is not None))
        assert all(r == runs[0] for r in runs[1:])
        same_planes(pl, wpl, entry)
        same_cloud(got, wp, wc, entry)


# ---- 6. history: poisoned buffers, other calls on the same engine, the stage record ---------------------------------------------
def _icp(e, ns, nt, entry="host"):
    i = IR.SHAPE_CASES.index((ns, nt))
    src, ds, tgt, dt, tn = IR.case_input(i)
    w = IR.case_want(i, True, 1)
    T, fit, rmse, corr, d2, hist, st = e.register_icp_host(src, ds, tgt, dt, tn, IR.R_CASE, (0, 0, 0), None, 1, IR.SHAPE_ITERATIONS)
    assert np.array_equal(corr, w["corr"]) and st.tolist() == w["stats"].tolist() and np.array_equal(T, w["T"])


def _voxel(e, i):
    xyz, disp, col = VR.case_input(i)
    H, W, v, o, mp = VR.SHAPE_CASES[i]
    w = VR.case_want(i)
    p, c, cnt, noor = e.voxel_downsample_host(xyz, disp, col, v, o, mp, return_counts=True)
    assert np.array_equal(u32(p), u32(w["points"])) and np.array_equal(c, w["colors"]) and np.array_equal(cnt, w["counts"])


def test_a_long_lived_engine_from_poisoned_buffers():
    """integrations and extractions at changing sizes interleaved with registration and voxel-grid calls on one engine whose buffers
    start as 0xA5 / 0x7F"""
    e = Engine(P16)

    def tsdf(i, entry):
        case = TR.cases()[i]
        pl = TR.empty(case[0], case[4])
        for k, (wpl, wst, wp, wc) in enumerate(want_case(i)):
            a = TR.case_input(case, seed=5 * k)
            assert integrate(e, entry, a, pl).tolist() == wst.tolist(), (i, entry, k)
            same_planes(pl, wpl, (i, entry, k))
        same_cloud(extract(e, entry, a, pl), wp, wc, (i, entry))
    try:
        for byte in (0xA5, 0x7F):
            e.set_option(_lib.SGM_OPT_POISON, byte)      # fills every buffer the engine owns and arms the same for new ones
            tsdf(14, "host")
            _icp(e, 257, 300)                            # xyz and f32 are shared with every host entry
            tsdf(5, "device")
            _voxel(e, 4)                                 # ... and cpts, crgb with the compactions
            tsdf(15, "host")
            e.set_option(_lib.SGM_OPT_POISON, byte)
            tsdf(0, "host")
            _icp(e, 1000, 5000)
            tsdf(16, "device")
            e.trim()                                     # gives the staged planes, the counts and the offsets back
            tsdf(11, "host")
            _voxel(e, 5)
            tsdf(12, "host")
    finally:
        e.set_option(_lib.SGM_OPT_POISON, -1)


def test_the_profile_record_names_the_stages():
    e = Engine(P16)
    i = 15
    a = TR.case_input(TR.cases()[i])
    wpl, wst, wp, wc = want_case(i)[0]
    try:
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        for entry in ("host", "device"):
            for stats, launches in ((True, 2), (False, 1)):
                pl = TR.empty(a["dims"])
                integrate(e, entry, a, pl, stats=stats)
                same_planes(pl, wpl, entry)
                assert [(n, k) for n, ms, k in e.stage_times()] == [("tsdf_integrate", launches), ("_wall", 0)]
            got = extract(e, entry, a, pl, cap=wp.shape[0])
            assert [(n, k) for n, ms, k in e.stage_times()] == [(n, 1) for n in _lib.TSDF_STAGES[1:]] + [("_wall", 0)]
            assert all(ms >= 0 for n, ms, k in e.stage_times())
            same_cloud(got, wp, wc, entry)
            assert extract(e, entry, a, pl, cap=0)[0] == wp.shape[0]
            assert [n for n, ms, k in e.stage_times()] == ["tsdf_count", "tsdf_scan", "_wall"]          # a call that only counts
    finally:
        e.set_option(_lib.SGM_OPT_PROFILE, 0)


def test_refusals_leave_everything_untouched_and_the_engine_usable(eng):
    i = 15
    a = TR.case_input(TR.cases()[i])
    wpl, wst, wp, wc = want_case(i)[0]
    pl = tuple(x.copy() for x in wpl)
    for kw, msg in ((dict(front=0), "front"), (dict(tau=F32(0)), "sdf_trunc"), (dict(vs=F32(np.nan)), "voxel_size"),
                    (dict(colors=None), "rgb_sum and colors"), (dict(ext=np.diag([1.0, 1, 1, 2])), "last row"),
                    (dict(cam=(1, np.nan, 1, 1)), "camera"), (dict(origin=np.array([0, np.inf, 0], F32)), "origin"),
                    (dict(dims=(40, 32, 4097)), "dimension")):
        for entry in ("host", "device"):
            with pytest.raises(sgm.error, match="sgm_tsdf_integrate.*" + msg):
                integrate(eng, entry, dict(a, **kw), pl)
            same_planes(pl, wpl, (kw, entry))
    with pytest.raises(sgm.error, match="sgm_tsdf_integrate.*max_depth"):
        integrate(eng, "host", a, pl, max_depth=0.0)
    for entry in ("host", "device"):
        with pytest.raises(sgm.error, match="sgm_tsdf_extract_points.*min_weight"):
            extract(eng, entry, a, pl, min_weight=0, cap=4)
    with pytest.raises(sgm.error, match="sgm_tsdf_extract_points.*rgb_sum"):        # colours asked of a volume without colour sums
        eng.tsdf_extract_host(a["dims"], a["vs"], a["origin"], pl[0], pl[1], None, 1, np.zeros((4, 3), F32), np.zeros((4, 3), np.uint8))
    same_planes(pl, wpl, "after the refusals")
    same_cloud(extract(eng, "device", a, pl), wp, wc, "after the refusals")


def test_the_compaction_and_the_voxel_grid_are_unchanged(eng):
    xyz, disp, col = VR.case_input(5)
    mask = np.isfinite(xyz[..., 0]) & (disp > 0)
    a = TR.case_input(TR.cases()[15])

    def others():
        p, c = eng.compact_points_host(xyz, disp, col)
        assert np.array_equal(u32(p), u32(xyz[mask])) and np.array_equal(c, col[mask])
        _voxel(eng, 5)
        _voxel(eng, 3)
    others()
    pl = TR.empty(a["dims"])
    integrate(eng, "host", a, pl)
    others()
    same_cloud(extract(eng, "host", a, pl), *want_case(15)[0][2:], "between")
    others()


# ---- 7. the Python class ---------------------------------------------------------------------------------------------------------
def test_the_python_class_on_arrays_and_on_tensors():
    import torch
    case = ((40, 32, 24), (48, 64), 1, -1, True, True)
    frames = [TR.case_input(case, seed=s) for s in (0, 5)]
    a = frames[0]
    conf = (np.arange(48 * 64).reshape(48, 64) % 7).astype(np.uint8)
    want = TR.empty((40, 32, 24))
    wst = [TR.run_case(f, want)[1] for f in frames]
    masked = dict(frames[1], disp=np.where(conf >= 3, frames[1]["disp"], F32(0)))
    wst.append(TR.run_case(masked, want, max_depth=12.0)[1])
    wp, wc = TR.extract((40, 32, 24), a["vs"], a["origin"], *want, 2)
    for on_device in (False, True):
        vol = sgm.TSDFVolume(float(a["vs"]), 1.0, (40, 32, 24), origin=a["origin"], device=on_device)
        assert (vol.device is None) == (not on_device) and sgm.stereo._is_torch(vol.sum) == on_device
        up = (lambda x: torch.from_numpy(x).cuda()) if on_device else (lambda x: x)
        st0 = vol.integrate(up(a["xyz"]), up(a["colors"]), up(a["disp"]), a["cam"], a["ext"], front=-1, return_stats=True)
        assert vol.integrate(up(frames[1]["xyz"]), frames[1]["colors"], up(frames[1]["disp"]), a["cam"], a["ext"]) is None      # front found
        st2 = vol.integrate(frames[1]["xyz"], up(frames[1]["colors"]), frames[1]["disp"], a["cam"], a["ext"], max_depth=12.0, confidence=conf,
                            min_confidence=3, return_stats=True)
        assert list(st0.values()) == wst[0][:7].tolist() and list(st2.values()) == wst[2][:7].tolist() and tuple(st0) == TR.STATS
        host = lambda x: x.cpu().numpy() if on_device else x
        assert np.array_equal(host(vol.sum).reshape(-1), want[0]) and np.array_equal(host(vol.weight).reshape(-1), want[1])
        assert np.array_equal(host(vol.rgb_sum).reshape(3, -1).view(np.uint32), want[2])
        p, c = vol.extract_point_cloud(2)
        assert (sgm.stereo._is_torch(p), sgm.stereo._is_torch(c)) == (on_device, on_device)
        assert np.array_equal(u32(host(p)), u32(wp)) and np.array_equal(host(c), wc) and wp.shape[0] > 500
        plain = sgm.TSDFVolume(float(a["vs"]), 1.0, (40, 32, 24), origin=a["origin"], color=False, device=on_device)
        plain.integrate(up(a["xyz"]), None, None, a["cam"], a["ext"])
        ref = TR.empty((40, 32, 24), False)
        TR.run_case(dict(a, disp=None, colors=None), ref)
        assert plain.rgb_sum is None and np.array_equal(host(plain.weight).reshape(-1), ref[1]) and plain.extract_point_cloud()[1] is None
        vol.reset()
        assert not host(vol.weight).any() and vol.extract_point_cloud()[0].shape == (0, 3)
    assert sgm.TSDFVolume(0.5, 1.0, (2, 2, 2)).device is not None          # the default where a GPU is present


# ---- 8. frames from the pipeline -------------------------------------------------------------------------------------------------
def test_two_270_x_480_frames_from_the_pipeline_under_the_rigs_motion():
    """two synthetic pairs of one scene geometry, each through sgm_pipeline_device, the second cloud expressed in the frame of a rig
    moved by a known motion (as in tests/test_gpu_icp.py); both integrated under their extrinsics -- the identity and the rig's
    motion -- with the camera of the notebook's Q, which looks down NEGATIVE Z, and extracted: equal to the reference"""
    import torch
    H, W, D = 270, 480, 64
    e = Engine(U.params(D, 5, 0, 1))
    Q = synth.default_Q(W)
    frames = []
    for seed in (5, 6):
        left, right = synth.make_pair(H, W, D, seed=seed)[:2]
        ta, tb = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        dd = torch.empty((H, W), dtype=torch.int16, device="cuda")
        df = torch.empty((H, W), dtype=torch.float32, device="cuda")
        dx = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, Q, dd.data_ptr(), df.data_ptr(), dx.data_ptr())
        e.synchronize()
        frames.append((dx.cpu().numpy(), df.cpu().numpy(), np.repeat(left[..., None], 3, axis=2)))
    (xyz, disp, col), (xyz_b, disp_b, col_b) = frames
    ok = np.isfinite(xyz).all(axis=2) & (disp > 0)
    assert (xyz[..., 2][ok] < 0).all()
    cam, front = sgm.camera_from_Q(Q)
    assert front == -1
    scale = float(np.median(np.abs(xyz[..., 2][ok])))
    rig = IR.rigid((0.2, 1.0, 0.1), 0.7, (0.012 * scale, -0.006 * scale, 0.008 * scale))
    xyz2 = sgm.transform_points(xyz_b, rig)                    # the second reconstruction in the moved rig's frame: world -> camera 2 is rig
    lo, hi = np.percentile(xyz[ok], 10, axis=0), np.percentile(xyz[ok], 90, axis=0)
    dims = (96, 64, 48)
    vs = F32(max((hi - lo) / np.array(dims)))
    origin = (0.5 * (lo + hi) - 0.5 * np.array(dims) * float(vs)).astype(F32)
    tau = F32(4 * vs)
    want = TR.empty(dims)
    wst = [TR.integrate(dims, vs, tau, origin, *want, xyz, disp, col, cam, front, EYE),
           TR.integrate(dims, vs, tau, origin, *want, xyz2, disp_b, col_b, cam, front, rig)]
    wp, wc = TR.extract(dims, vs, origin, *want, 2)
    vol = sgm.TSDFVolume(float(vs), float(tau), dims, origin=origin)
    st = [vol.integrate(torch.from_numpy(xyz).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(disp).cuda(), cam, None, return_stats=True),
          vol.integrate(torch.from_numpy(xyz2).cuda(), torch.from_numpy(col_b).cuda(), torch.from_numpy(disp_b).cuda(), cam, rig, return_stats=True)]
    assert [list(s.values()) for s in st] == [w[:7].tolist() for w in wst]
    assert np.array_equal(vol.sum.cpu().numpy().reshape(-1), want[0]) and np.array_equal(vol.weight.cpu().numpy().reshape(-1), want[1])
    assert np.array_equal(vol.rgb_sum.cpu().numpy().reshape(3, -1).view(np.uint32), want[2])
    p, c = vol.extract_point_cloud(2)
    print("pipeline frames: updated", st[0]["updated"], st[1]["updated"], "seen twice", int((want[1] == 2).sum()), "crossings", wp.shape[0])
    assert np.array_equal(u32(p.cpu().numpy()), u32(wp)) and np.array_equal(c.cpu().numpy(), wc)
    assert st[0]["updated"] > 20000 and st[1]["updated"] > 20000 and (want[1] == 2).sum() > 10000 and wp.shape[0] > 1000


# ---- 9. planes past 2^31 bytes ---------------------------------------------------------------------------------------------------
def test_a_volume_whose_planes_pass_two_gib(eng):
    """1024 x 1024 x 513 without colour: slab 512 of each plane begins at byte 2^31.  One frame integrated; slab 0, and slabs 511 and 512
    on both sides of that byte, against the reference's z-range form.  Then an extraction from planes this test fills itself --
    non-zero in slabs 0, 511 and 512 only -- equal to the reference in full (the z edges between 511 and 512 cross the byte)."""
    import torch
    dims = (1024, 1024, 513)
    nxy, V = 1024 * 1024, 1024 * 1024 * 513
    assert nxy * 512 * 4 == 1 << 31 and V <= 1 << 30
    H, W = 48, 64
    xyz, disp, _ = TR.make_frame(H, W, 1, seed=2, noise=0.05)
    vs, tau = F32(10.0 / 1024), F32(4.0)
    origin = np.array([-5.0, -5.0, TR.DEPTH - 0.5 * 513 * float(vs)], F32)
    cam = TR.camera_for(H, W)
    ts = torch.zeros(V, dtype=torch.int32, device="cuda")
    tw = torch.zeros(V, dtype=torch.int32, device="cuda")
    tx, td = dev(xyz), dev(disp)
    torch.cuda.synchronize()
    st = eng.tsdf_integrate_device(dims, vs, tau, origin, ts.data_ptr(), tw.data_ptr(), None, tx.data_ptr(), td.data_ptr(), None, H, W, cam, 1, EYE,
                                   stats=True)
    eng.synchronize()
    assert int(st[:6].sum() - st[1]) == V and st[0] > V // 4
    for k in (0, 511, 512):
        ref = TR.empty((1024, 1024, 1), False)
        wst = TR.integrate(dims, vs, tau, origin, ref[0], ref[1], None, xyz, disp, None, cam, 1, EYE, z0=k, z1=k + 1)
        assert wst[0] > 100000
        assert np.array_equal(ts[k * nxy:(k + 1) * nxy].cpu().numpy(), ref[0]) and np.array_equal(tw[k * nxy:(k + 1) * nxy].cpu().numpy(), ref[1]), k
    assert int(tw.sum(dtype=torch.int64)) == int(st[0])
    # the extraction: sparse random slabs
    ts.zero_()
    tw.zero_()
    hs, hw = np.zeros(V, np.int32), np.zeros(V, np.int32)        # (untouched pages cost nothing)
    rng = np.random.default_rng(11)
    for k in (0, 511, 512):
        on = rng.random(nxy) < 0.125
        hw[k * nxy:(k + 1) * nxy] = np.where(on, rng.integers(1, 4, nxy), 0)
        hs[k * nxy:(k + 1) * nxy] = np.where(on, rng.integers(-30000, 30000, nxy), 0)
        ts[k * nxy:(k + 1) * nxy] = torch.from_numpy(hs[k * nxy:(k + 1) * nxy]).cuda()
        tw[k * nxy:(k + 1) * nxy] = torch.from_numpy(hw[k * nxy:(k + 1) * nxy]).cuda()
    wp, _, axes = TR.extract(dims, vs, origin, hs, hw, None, 1, with_axis=True)
    n = wp.shape[0]
    assert n > 20000 and all((axes == a).sum() > 1000 for a in range(3))
    torch.cuda.synchronize()
    assert eng.tsdf_extract_device(dims, vs, origin, ts.data_ptr(), tw.data_ptr(), None, 1) == n
    tp = torch.full((n + 5, 3), float(MARK), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert eng.tsdf_extract_device(dims, vs, origin, ts.data_ptr(), tw.data_ptr(), None, 1, n + 5, tp.data_ptr()) == n
    got = tp.cpu().numpy()
    assert np.array_equal(u32(got[:n]), u32(wp)) and (got[n:] == MARK).all()


# ---- 10. guarded buffers ---------------------------------------------------------------------------------------------------------
def test_the_cases_with_every_buffer_guarded():
    """(the same cases ran in the plain mode above)"""
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tsdf_guard_child.py")], capture_output=True, text=True, env=env,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"TSDF_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) >= len(TR.cases()), tail
