"""Voxel-grid downsampling on the device (needs an MI355X): sgm_voxel_downsample, sgm_voxel_downsample_device,
Engine.voxel_downsample_host / _device, sgm.voxel_down_sample.

Yardstick: tests/voxel_ref.py -- the definition of include/sgm_hip_voxel.h in numpy, voxels grouped with np.unique -- bit for bit:
points, colours, counts and both totals.  Every output is pre-filled with a marker, so rows past n_voxels are seen untouched, and
every input is checked unmodified."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import parity_util as U
import voxel_ref as VR
import stereo_reconstruction_cv_amd as sgm
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = dict(numDisparities=16)
NCASE = len(VR.SHAPE_CASES)
TIGHT, OTHER = _lib.SGM_DBG_VOXEL_TIGHT_TABLE, _lib.SGM_DBG_VOXEL_OTHER_REDUCTION
MARK_F, MARK_B, MARK_C = np.float32(-77.25), 177, 0xDEADBEEF


@pytest.fixture(scope="module")
def eng():
    return Engine(P16)


@functools.lru_cache(maxsize=None)
def layered():
    """the 48 x 320 layered cloud as lists, shared and read-only"""
    xyz, disp, col = VR.layered_cloud(48, 320, 704)
    out = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)
    for a in out:
        a.setflags(write=False)
    return out


def host(e, xyz, disp, col, v, o=(0, 0, 0), mp=1, counts=True):
    """the host entry called on marked outputs of n rows: (points, colors, counts, n_voxels, n_out_of_range), whole arrays"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    keep = [xyz.copy(), None if disp is None else disp.copy(), None if col is None else col.copy()]
    pts = np.full((max(n, 1), 3), MARK_F, np.float32)
    rgb = None if col is None else np.full((max(n, 1), 3), MARK_B, np.uint8)
    cnt = np.full(max(n, 1), MARK_C, np.uint32) if counts else None
    org = np.asarray(o, np.float32)
    nv, noor = C.c_int64(-5), C.c_int64(-5)
    at = lambda a: None if a is None else a.ctypes.data
    rc = _lib.load().sgm_voxel_downsample(e._h, xyz.ctypes.data, at(disp), at(col), n, float(v), org.ctypes.data, int(mp), pts.ctypes.data,
                                          at(rgb), at(cnt), C.byref(nv), C.byref(noor))
    assert rc == 0, _lib.last_error()
    assert np.array_equal(xyz, keep[0], equal_nan=True) and (disp is None or np.array_equal(disp, keep[1], equal_nan=True))
    assert col is None or np.array_equal(col, keep[2])
    return pts, rgb, cnt, nv.value, noor.value


def device(e, xyz, disp, col, v, o=(0, 0, 0), mp=1, counts=True):
    """the same through the device entry, every array a tensor of its own"""
    import torch
    dev = torch.device("cuda", e.device)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    dx, dd, dc = up(xyz), up(disp), up(col)
    pts = torch.full((n, 3), float(MARK_F), dtype=torch.float32, device=dev)
    rgb = None if col is None else torch.full((n, 3), MARK_B, dtype=torch.uint8, device=dev)
    cnt = torch.from_numpy(np.full(n, MARK_C, np.uint32).view(np.int32)).to(dev) if counts else None
    p = lambda t: None if t is None else t.data_ptr()
    torch.cuda.synchronize()
    nv, noor = e.voxel_downsample_device(p(dx), p(dd), p(dc), n, v, o, mp, p(pts), p(rgb), p(cnt))
    e.synchronize()
    assert np.array_equal(dx.cpu().numpy(), xyz, equal_nan=True) and (disp is None or np.array_equal(dd.cpu().numpy(), disp, equal_nan=True))
    assert col is None or np.array_equal(dc.cpu().numpy(), col)
    back = lambda t: None if t is None else t.cpu().numpy()
    return back(pts), back(rgb), None if cnt is None else back(cnt).view(np.uint32), nv, noor


def same(got, want, what=""):
    """bit for bit against a reference result, and the rows behind it untouched"""
    pts, rgb, cnt, nv, noor = got
    m = want["n_voxels"]
    assert (nv, noor) == (m, want["n_out_of_range"]), (what, nv, noor, m, want["n_out_of_range"])
    assert pts.dtype == np.float32 and np.array_equal(pts[:m].view(np.uint32), want["points"].view(np.uint32)), \
        (what, int((pts[:m].view(np.uint32) != want["points"].view(np.uint32)).sum()))
    assert (pts[m:] == MARK_F).all(), what
    if rgb is not None:
        assert rgb.dtype == np.uint8 and np.array_equal(rgb[:m], want["colors"]) and (rgb[m:] == MARK_B).all(), what
    if cnt is not None:
        assert cnt.dtype == np.uint32 and np.array_equal(cnt[:m], want["counts"]) and (cnt[m:] == MARK_C).all(), what


def both(e, xyz, disp, col, v, o=(0, 0, 0), mp=1, want=None, what=""):
    if want is None:
        want = VR.voxel_downsample(np.asarray(xyz, np.float32).reshape(-1, 3), disp, col, v, o, mp)
    same(host(e, xyz, disp, col, v, o, mp), want, (what, "host"))
    same(device(e, xyz, disp, col, v, o, mp), want, (what, "device"))
    return want


# ---- 1. shapes, through both entries, with and without colours, counts and disp -----------------------------------------------------
@pytest.mark.parametrize("i", range(NCASE))
def test_shapes_through_both_entries(eng, i):
    H, W, v, o, mp = VR.SHAPE_CASES[i]
    xyz, disp, col = (a.reshape(-1, a.shape[-1]) if a.ndim == 3 else a.reshape(-1) for a in VR.case_input(i))
    for with_disp in (True, False):
        for with_col in (True, False):
            want = VR.case_want(i, with_disp, with_col)
            for fn in (host, device):
                got = fn(eng, xyz, disp if with_disp else None, col if with_col else None, v, o, mp, counts=with_col != with_disp)
                same(got, want, (H, W, fn.__name__, with_disp, with_col))
    assert VR.case_want(i)["n_voxels"] > 0


def test_colours_given_but_not_asked_for_are_ignored(eng):
    xyz, disp, col = layered()
    import torch
    n = xyz.shape[0]
    dx, dc = torch.from_numpy(np.array(xyz)).cuda(), torch.from_numpy(np.array(col)).cuda()
    pts = torch.full((n, 3), float(MARK_F), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    nv, noor = eng.voxel_downsample_device(dx.data_ptr(), None, dc.data_ptr(), n, 0.05, (0, 0, 0), 1, pts.data_ptr(), None, None)
    same((pts.cpu().numpy(), None, None, nv, noor), VR.voxel_downsample(xyz, None, None, 0.05))


# ---- 2. extremes at 48 x 320 -----------------------------------------------------------------------------------------------------------
def test_every_point_invalid(eng):
    xyz, disp, col = layered()
    n = xyz.shape[0]
    want = both(eng, xyz, np.zeros(n, np.float32), col, 0.05, what="disp 0")
    assert want["n_voxels"] == 0
    bad = np.array(xyz)
    bad[np.arange(n), np.arange(n) % 3] = np.nan
    assert both(eng, bad, None, col, 0.05, what="nan")["n_voxels"] == 0
    assert both(eng, np.full((n, 3), 3e38, np.float32), None, None, 1.0, what="all out of range")["n_out_of_range"] == n


def test_every_point_in_one_voxel(eng):
    """a huge voxel: every atomic of the call lands on one slot"""
    xyz, disp, col = layered()
    want = both(eng, xyz, disp, col, 1.0e6, o=(-5.0e5, -5.0e5, -5.0e5), what="one voxel")
    assert want["n_voxels"] == 1 and want["counts"][0] > 12000


def test_every_point_in_a_voxel_of_its_own(eng):
    """a tiny voxel: as many slots in use as points"""
    xyz, disp, col = layered()
    want = both(eng, xyz, disp, col, 1.0e-5, what="own voxels")
    assert want["n_voxels"] > 12000 and (want["counts"] == 1).mean() > 0.99 and want["n_out_of_range"] == 0


def test_negative_coordinates_on_all_axes(eng):
    xyz, disp, col = layered()
    neg = -np.abs(np.array(xyz)) - np.float32(0.37)
    want = both(eng, neg, disp, col, 0.05, what="negative")
    assert want["n_voxels"] > 300 and (want["points"] < 0).all()      # (folding the cloud into one octant halves its voxels)


def test_the_saturation_point(eng):
    pts = np.array([[-1e-10, 0.5, 0.5], [0.25, -1e-10, 0.5], [-1e-10, -1e-10, -1e-10], [0.5, 0.5, 0.5]], np.float32)
    for v in (1.0, 0.05):
        want = both(eng, pts, None, None, v, what=("saturation", v))
        assert want["n_voxels"] == 4 and want["points"][0, 0] == np.float32(-1.0 / 65536) * np.float32(v)


def test_out_of_range_points_among_ordinary_ones(eng):
    xyz, disp, col = layered()
    far = np.array(xyz)
    far[5::7, 0] = 3.0e5          # g = 6e6 at v = 0.05
    far[3::11, 2] = -1.0e30
    far[100, 1] = np.float32(2 ** 20 * 0.05)
    want = both(eng, far, disp, col, 0.05, what="out of range")
    assert want["n_out_of_range"] > 2500 and want["n_voxels"] > 500


def test_a_nonzero_origin(eng):
    xyz, disp, col = layered()
    want = both(eng, xyz, disp, col, 0.04, o=(0.013, -2.5, 100.0), what="origin")
    assert want["n_voxels"] > 500


@pytest.mark.parametrize("mp", [1, 2, 5])
def test_min_points(eng, mp):
    xyz, disp, col = layered()
    want = both(eng, xyz, disp, col, 0.05, mp=mp, what=("min_points", mp))
    assert want["n_voxels"] > 100 and (want["counts"] >= mp).all() and (np.diff(want["first"]) > 0).all()


# ---- 3. the two debug bits ---------------------------------------------------------------------------------------------------------------
def test_the_tight_table_gives_the_same_bits():
    """load exactly 1.0: 64 x 64 points, each in a voxel of its own, in 4096 slots -- the longest probe chains; then the layered
    cloud in the smallest table that holds it"""
    e = Engine(P16)
    g = np.stack(np.meshgrid(np.arange(64), np.arange(64), indexing="ij"), axis=2).reshape(-1, 2)
    own = np.concatenate([g, (g[:, :1] * 7 + g[:, 1:]) % 5], axis=1).astype(np.float32) + np.float32(0.5)
    xyz, disp, col = layered()
    plain = [host(e, own, None, None, 1.0), host(e, xyz, disp, col, 0.05), host(e, xyz, disp, col, 1.0e-5)]
    try:
        e.set_option(_lib.SGM_OPT_DEBUG, TIGHT)
        want = both(e, own, None, None, 1.0, what="tight 64 x 64")
        assert want["n_voxels"] == 4096 and (want["counts"] == 1).all()
        both(e, xyz, disp, col, 0.05, what="tight layered")
        both(e, xyz, disp, col, 1.0e-5, what="tight layered, own voxels")
        tight = [host(e, own, None, None, 1.0), host(e, xyz, disp, col, 0.05), host(e, xyz, disp, col, 1.0e-5)]
        e.set_option(_lib.SGM_OPT_DEBUG, TIGHT | OTHER)
        both(e, own, None, None, 1.0, want=want, what="tight, other reduction")
    finally:
        e.set_option(_lib.SGM_OPT_DEBUG, 0)
    for a, b in zip(plain, tight):
        assert a[3:] == b[3:] and all(x is None or np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[:3], b[:3]))


def test_the_other_reduction_gives_the_same_bits():
    e = Engine(P16)
    xyz, disp, col = layered()
    cases = [(xyz, disp, col, 0.05, (0, 0, 0), 1), (xyz, disp, col, 1.0e6, (-5.0e5,) * 3, 1), (xyz, None, None, 0.2, (0, 0, 0), 2),
             (xyz, disp, col, 1.0e-5, (0, 0, 0), 1)]
    wants = [both(e, *c[:5], mp=c[5], what="default") for c in cases]
    try:
        e.set_option(_lib.SGM_OPT_DEBUG, OTHER)
        for c, w in zip(cases, wants):
            both(e, *c[:5], mp=c[5], want=w, what="other reduction")
    finally:
        e.set_option(_lib.SGM_OPT_DEBUG, 0)


# ---- 4. determinism, history, poison -----------------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bits(eng):
    xyz, disp, col = layered()
    a, b = device(eng, xyz, disp, col, 0.03, mp=2), device(eng, xyz, disp, col, 0.03, mp=2)
    assert a[3:] == b[3:] and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[:3], b[:3]))
    same(a, VR.voxel_downsample(xyz, disp, col, 0.03, min_points=2))


def test_results_do_not_depend_on_what_the_engine_did_before():
    e = Engine(P16)
    def run(i, fn):
        H, W, v, o, mp = VR.SHAPE_CASES[i]
        xyz, disp, col = VR.case_input(i)
        same(fn(e, xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3), v, o, mp), VR.case_want(i), (i, fn.__name__))
    big, small = 5, 3                       # 97 x 331, then 3 x 257
    run(small, host)
    run(big, device)
    run(small, device)                      # a smaller cloud in the larger table
    run(big, host)
    e.trim()                                # gives the table back; it returns on the next call
    run(small, device)
    try:
        for byte in (0xA5, 0x7F):
            e.set_option(_lib.SGM_OPT_POISON, byte)      # fills every buffer the engine owns and arms the same for new ones
            run(small, host)
            e.set_option(_lib.SGM_OPT_POISON, byte)
            run(big, device)
            run(small, device)
    finally:
        e.set_option(_lib.SGM_OPT_POISON, -1)


def test_the_profile_record_names_the_stages():
    e = Engine(P16)
    xyz, disp, col = layered()
    try:
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        same(device(e, xyz, disp, col, 0.05), VR.voxel_downsample(xyz, disp, col, 0.05))
        st = {n: launches for n, ms, launches in e.stage_times()}
        assert st == {"voxel_count": 1, "voxel_clear": 1, "voxel_insert": 1, "voxel_heads": 3, "_wall": 0}, st
    finally:
        e.set_option(_lib.SGM_OPT_PROFILE, 0)


# ---- 5. one mid-size frame from the pipeline -----------------------------------------------------------------------------------------
def test_one_1080p_frame_from_the_pipeline():
    """1080 x 1920 through sgm_pipeline_device, then the device entry on the resident XYZ image at two voxel sizes: two million
    points from every compute unit at once on one table"""
    import torch
    H, W, D = 1080, 1920, 128
    a, b = synth.make_pair(H, W, D, seed=5)[:2]
    e = Engine(U.params(D, 5, 0, 1))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dd = torch.empty((H, W), dtype=torch.int16, device="cuda")
    df = torch.empty((H, W), dtype=torch.float32, device="cuda")
    dx = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    rgb = torch.from_numpy(np.repeat(a[:, :, None], 3, axis=2) ^ np.array([0, 85, 170], np.uint8)).cuda()
    torch.cuda.synchronize()
    e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, synth.default_Q(W), dd.data_ptr(), df.data_ptr(), dx.data_ptr())
    e.synchronize()
    xyz, disp, col = dx.cpu().numpy().reshape(-1, 3), df.cpu().numpy().reshape(-1), rgb.cpu().numpy().reshape(-1, 3)
    n = H * W
    ok = np.isfinite(xyz).all(axis=1) & (disp > 0)
    assert ok.mean() > 0.3
    z = float(np.median(np.abs(xyz[ok, 2])))
    pts = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    oc = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    ok_ = torch.empty(n, dtype=torch.int32, device="cuda")
    for v, mp in ((z / 400, 1), (z / 30, 2)):
        want = VR.voxel_downsample(xyz, disp, col, v, min_points=mp)
        pts.fill_(float(MARK_F)), oc.fill_(MARK_B), ok_.fill_(-1)
        torch.cuda.synchronize()
        nv, noor = e.voxel_downsample_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), n, v, (0, 0, 0), mp, pts.data_ptr(), oc.data_ptr(),
                                             ok_.data_ptr())
        got_c = ok_.cpu().numpy().view(np.uint32)
        assert (nv, noor) == (want["n_voxels"], want["n_out_of_range"]) and nv > 1000
        assert np.array_equal(pts[:nv].cpu().numpy().view(np.uint32), want["points"].view(np.uint32))
        assert np.array_equal(oc[:nv].cpu().numpy(), want["colors"]) and np.array_equal(got_c[:nv], want["counts"])
        assert bool((pts[nv:] == float(MARK_F)).all()) and bool((oc[nv:] == MARK_B).all()) and (got_c[nv:] == 0xFFFFFFFF).all()
    assert np.array_equal(dx.cpu().numpy().reshape(-1, 3), xyz, equal_nan=True)


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched_and_the_engine_usable(eng):
    L = _lib.load()
    xyz, disp, col = layered()
    xyz, col = np.array(xyz[:100]), np.array(col[:100])
    n = 100
    pts, rgb, cnt = np.full((n, 3), MARK_F, np.float32), np.full((n, 3), MARK_B, np.uint8), np.full(n, MARK_C, np.uint32)
    nv, noor = C.c_int64(-5), C.c_int64(-6)
    org, nan_org = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(0, float("nan"), 0)
    X, Cc, P, R, K = xyz.ctypes.data, col.ctypes.data, pts.ctypes.data, rgb.ctypes.data, cnt.ctypes.data
    NV, NO = C.byref(nv), C.byref(noor)
    bad = [
        (None, X, None, Cc, n, 0.05, org, 1, P, R, K, NV, NO), (eng._h, None, None, Cc, n, 0.05, org, 1, P, R, K, NV, NO),
        (eng._h, X, None, Cc, n, 0.05, org, 1, None, R, K, NV, NO), (eng._h, X, None, Cc, n, 0.05, org, 1, P, R, K, None, NO),
        (eng._h, X, None, Cc, -1, 0.05, org, 1, P, R, K, NV, NO),
        (eng._h, X, None, Cc, n, 0.0, org, 1, P, R, K, NV, NO), (eng._h, X, None, Cc, n, -1.0, org, 1, P, R, K, NV, NO),
        (eng._h, X, None, Cc, n, float("nan"), org, 1, P, R, K, NV, NO), (eng._h, X, None, Cc, n, float("inf"), org, 1, P, R, K, NV, NO),
        (eng._h, X, None, Cc, n, 1e-45, org, 1, P, R, K, NV, NO),
        (eng._h, X, None, Cc, n, 0.05, nan_org, 1, P, R, K, NV, NO), (eng._h, X, None, Cc, n, 0.05, None, 1, P, R, K, NV, NO),
        (eng._h, X, None, Cc, n, 0.05, org, 0, P, R, K, NV, NO), (eng._h, X, None, Cc, n, 0.05, org, -3, P, R, K, NV, NO),
        (eng._h, X, None, None, n, 0.05, org, 1, P, R, K, NV, NO),
    ]
    for fn in (L.sgm_voxel_downsample, L.sgm_voxel_downsample_device):
        for args in bad:
            assert fn(*args) == -1, args                                   # SGM_ERR_INVALID_ARG
            assert b"sgm_voxel_downsample" in L.sgm_last_error()
        assert fn(eng._h, X, None, Cc, 1 << 24, 0.05, org, 1, P, R, K, NV, NO) == -4     # SGM_ERR_UNSUPPORTED: before anything is read
        assert b"2^24" in L.sgm_last_error()
    assert (pts == MARK_F).all() and (rgb == MARK_B).all() and (cnt == MARK_C).all() and (nv.value, noor.value) == (-5, -6)
    # n = 0 succeeds with 0 voxels
    for fn in (L.sgm_voxel_downsample, L.sgm_voxel_downsample_device):
        nv.value, noor.value = -5, -6
        assert fn(eng._h, X, None, None, 0, 0.05, org, 1, P, None, None, NV, NO) == 0 and (nv.value, noor.value) == (0, 0)
        assert fn(eng._h, X, None, None, 0, 0.05, org, 1, P, None, None, NV, None) == 0
    assert (pts == MARK_F).all()
    a, b, c = layered()
    both(eng, a, b, c, 0.05, what="after the refusals")


# ---- 7. the existing paths ---------------------------------------------------------------------------------------------------------------
def test_the_compaction_is_unchanged_after_a_voxel_call():
    import torch
    e = Engine(P16)
    xyz, disp, col = VR.layered_cloud(97, 331, 9)
    mask = ~np.isnan(xyz[:, :, 0]) & ~np.isinf(xyz[:, :, 0]) & (disp > 0)
    both(e, xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3), 0.05)
    p, c = e.compact_points_host(xyz, disp, col)
    assert np.array_equal(p.view(np.uint32), xyz[mask].view(np.uint32)) and np.array_equal(c, col[mask])
    n = disp.size
    dx, dd, dc = (torch.from_numpy(a).cuda() for a in (xyz, disp, col))
    op, oc = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    m = e.compact_points_device(dx.data_ptr(), dd.data_ptr(), dc.data_ptr(), n, op.data_ptr(), oc.data_ptr())
    assert m == int(mask.sum())
    assert np.array_equal(op[:m].cpu().numpy().view(np.uint32), xyz[mask].view(np.uint32)) and np.array_equal(oc[:m].cpu().numpy(), col[mask])
    sgm.voxel_down_sample(xyz, col, disp, 0.05)                    # ... and on the default engine, which valid_points uses
    p, c = sgm.valid_points(xyz, col, disp)
    assert np.array_equal(p.view(np.uint32), xyz[mask].view(np.uint32)) and np.array_equal(c, col[mask])


# ---- 8. the Python surface -----------------------------------------------------------------------------------------------------------------
def test_voxel_down_sample_on_numpy_input():
    xyz, disp, col = VR.layered_cloud(48, 320, 31)
    want = VR.voxel_downsample(xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3), 0.05)
    p, c = sgm.voxel_down_sample(xyz, col, disp, 0.05)
    assert p.dtype == np.float32 and c.dtype == np.uint8
    assert np.array_equal(p.view(np.uint32), want["points"].view(np.uint32)) and np.array_equal(c, want["colors"])
    p, c, k = sgm.voxel_down_sample(xyz, col, disp, 0.05, return_counts=True)
    assert k.dtype == np.uint32 and np.array_equal(k, want["counts"]) and np.array_equal(p, want["points"])
    p, c = sgm.voxel_down_sample(xyz, None, disp, 0.05)
    assert c is None and np.array_equal(p, want["points"])
    # a list without a disparity map, another origin and a floor on the count
    lst = xyz.reshape(-1, 3)
    w2 = VR.voxel_downsample(lst, None, col.reshape(-1, 3), 0.08, (0.5, 0.5, 0.5), 3)
    p, c, k = sgm.voxel_down_sample(lst, col.reshape(-1, 3), None, 0.08, origin=(0.5, 0.5, 0.5), min_points=3, return_counts=True)
    assert np.array_equal(p.view(np.uint32), w2["points"].view(np.uint32)) and np.array_equal(c, w2["colors"]) and np.array_equal(k, w2["counts"])
    # with a confidence map: the mask of valid_points
    conf = np.random.default_rng(3).integers(0, 101, size=disp.shape).astype(np.uint8)
    w3 = VR.voxel_downsample(lst, np.where(conf >= 40, disp, np.float32(0)).reshape(-1), col.reshape(-1, 3), 0.05)
    p, c = sgm.voxel_down_sample(xyz, col, disp, 0.05, confidence=conf, min_confidence=40)
    assert w3["n_voxels"] < want["n_voxels"]
    assert np.array_equal(p.view(np.uint32), w3["points"].view(np.uint32)) and np.array_equal(c, w3["colors"])
    # an empty list
    p, c = sgm.voxel_down_sample(np.zeros((0, 3), np.float32), None, None, 0.05)
    assert p.shape == (0, 3) and c is None


# ---- 9. guarded buffers -------------------------------------------------------------------------------------------------------------------
def test_the_cases_with_every_buffer_guarded():
    """(the same cases ran in the plain mode above)"""
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "voxel_guard_child.py")], capture_output=True, text=True, env=env,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"VOXEL_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) >= 12, tail
