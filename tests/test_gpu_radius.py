"""Radius outlier removal on the device (needs an MI355X): sgm_radius_outlier, sgm_radius_outlier_device,
Engine.radius_outlier_host / _device, sgm.remove_radius_outlier.

Yardstick: tests/radius_ref.py -- the definition of include/sgm_hip_radius.h in numpy, over all pairs or over 27 cells -- bit for
bit: keep, counts, points, colours, index and both totals, through both entries.  Every output is pre-filled with a marker, so
rows past n_kept are seen untouched, and every input is checked unmodified."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mesh_ref as MR
import normals_ref as NR
import parity_util as U
import radius_ref as RR
import voxel_ref as VR
import stereo_reconstruction_cv_amd as sgm
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = dict(numDisparities=16)
NCASE = len(RR.SHAPE_CASES)
TIGHT, SOURCE = _lib.SGM_DBG_RADIUS_TIGHT_TABLE, _lib.SGM_DBG_RADIUS_SOURCE_ORDER
MARK_F, MARK_B, MARK_C, MARK_K = np.float32(-77.25), 177, 0xDEADBEEF, 99
ALL = ("keep", "counts", "points", "colors", "index")


@pytest.fixture(scope="module")
def eng():
    return Engine(P16)


@functools.lru_cache(maxsize=None)
def layered():
    """the 48 x 320 layered cloud as lists, shared and read-only"""
    return RR.layered_lists(48, 320, 704)


def host(e, xyz, disp, col, r, nb, mc=None, o=(0, 0, 0), outs=ALL):
    """the host entry called on marked outputs: a dict of whole arrays (None where not asked for), n_kept, n_out_of_range"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    before = [xyz.copy(), None if disp is None else np.array(disp), None if col is None else np.array(col)]
    m = max(n, 1)
    g = dict(keep=np.full(m, MARK_K, np.uint8) if "keep" in outs else None,
             counts=np.full(m, MARK_C, np.uint32) if "counts" in outs else None,
             points=np.full((m, 3), MARK_F, np.float32) if "points" in outs else None,
             colors=np.full((m, 3), MARK_B, np.uint8) if "colors" in outs and col is not None else None,
             index=np.full(m, MARK_C, np.uint32) if "index" in outs else None)
    org = np.asarray(o, np.float32)
    nk, noor = C.c_int64(-5), C.c_int64(-5)
    at = lambda a: None if a is None else a.ctypes.data
    rc = _lib.load().sgm_radius_outlier(e._h, xyz.ctypes.data, at(disp), at(col), n, float(r), org.ctypes.data, int(nb),
                                        int(nb if mc is None else mc), at(g["keep"]), at(g["counts"]), at(g["points"]), at(g["colors"]),
                                        at(g["index"]), C.byref(nk), C.byref(noor))
    assert rc == 0, _lib.last_error()
    assert np.array_equal(xyz, before[0], equal_nan=True) and (disp is None or np.array_equal(disp, before[1], equal_nan=True))
    assert col is None or np.array_equal(col, before[2])
    return dict(g, n=n, n_kept=nk.value, n_out_of_range=noor.value)


def device(e, xyz, disp, col, r, nb, mc=None, o=(0, 0, 0), outs=ALL):
    """the same through the device entry, every array a tensor of its own"""
    import torch
    dev = torch.device("cuda", e.device)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    dx, dd, dc = up(xyz), up(disp), up(col)
    m = max(n, 1)
    word = lambda: torch.from_numpy(np.full(m, MARK_C, np.uint32).view(np.int32)).to(dev)
    t = dict(keep=torch.full((m,), MARK_K, dtype=torch.uint8, device=dev) if "keep" in outs else None,
             counts=word() if "counts" in outs else None,
             points=torch.full((m, 3), float(MARK_F), dtype=torch.float32, device=dev) if "points" in outs else None,
             colors=torch.full((m, 3), MARK_B, dtype=torch.uint8, device=dev) if "colors" in outs and col is not None else None,
             index=word() if "index" in outs else None)
    p = lambda x: None if x is None else x.data_ptr()
    torch.cuda.synchronize()
    nk, noor = e.radius_outlier_device(p(dx), p(dd), p(dc), n, r, nb, mc, o, p(t["keep"]), p(t["counts"]), p(t["points"]), p(t["colors"]),
                                       p(t["index"]))
    e.synchronize()
    assert np.array_equal(dx.cpu().numpy(), xyz, equal_nan=True) and (disp is None or np.array_equal(dd.cpu().numpy(), disp, equal_nan=True))
    assert col is None or np.array_equal(dc.cpu().numpy(), col)
    g = {k: None if x is None else x.cpu().numpy() for k, x in t.items()}
    for k in ("counts", "index"):
        g[k] = None if g[k] is None else g[k].view(np.uint32)
    return dict(g, n=n, n_kept=nk, n_out_of_range=noor)


def same(got, want, what=""):
    """bit for bit against a reference result, and the rows behind n_kept untouched"""
    n, m = got["n"], want["n_kept"]
    assert (got["n_kept"], got["n_out_of_range"]) == (m, want["n_out_of_range"]), (what, got["n_kept"], got["n_out_of_range"], m)
    if got["keep"] is not None:
        assert got["keep"].dtype == np.uint8 and np.array_equal(got["keep"][:n], want["keep"]), (what, "keep")
    if got["counts"] is not None:
        bad = np.nonzero(got["counts"][:n] != want["counts"])[0]
        assert got["counts"].dtype == np.uint32 and bad.size == 0, (what, "counts", bad[:5], got["counts"][bad[:5]], want["counts"][bad[:5]])
    if got["points"] is not None:
        assert np.array_equal(got["points"][:m].view(np.uint32), want["points"].view(np.uint32)) and (got["points"][m:] == MARK_F).all(), what
    if got["colors"] is not None:
        assert np.array_equal(got["colors"][:m], want["colors"]) and (got["colors"][m:] == MARK_B).all(), what
    if got["index"] is not None:
        assert np.array_equal(got["index"][:m], want["index"]) and (got["index"][m:] == MARK_C).all(), what


def both(e, xyz, disp, col, r, nb, mc=None, o=(0, 0, 0), want=None, what=""):
    if want is None:
        want = RR.cells(np.asarray(xyz, np.float32).reshape(-1, 3), disp, col, r, nb, mc, o)
    same(host(e, xyz, disp, col, r, nb, mc, o), want, (what, "host"))
    same(device(e, xyz, disp, col, r, nb, mc, o), want, (what, "device"))
    return want


def bytes_of(g):
    return [None if g[k] is None else g[k].tobytes() for k in ALL] + [g["n_kept"], g["n_out_of_range"]]


# ---- 1. shapes, through both entries, with and without disp, colours and each optional output -------------------------------------
@pytest.mark.parametrize("i", range(NCASE))
def test_shapes_through_both_entries(eng, i):
    kind, a, b, r, nb, mc, o = RR.SHAPE_CASES[i]
    xyz, disp, col = RR.case_input(i)
    for with_disp in ((True, False) if disp is not None else (False,)):
        want = RR.case_want(i, with_disp)
        for fn in (host, device):
            same(fn(eng, xyz, disp if with_disp else None, col, r, nb, mc, o), want, (i, fn.__name__, with_disp))
    want = RR.case_want(i)
    for k, fn in zip(ALL, (host, device, host, device, host)):           # each output alone, and none at all
        same(fn(eng, xyz, disp, col, r, nb, mc, o, outs=(k,)), want, (i, "only", k))
    same(device(eng, xyz, disp, None, r, nb, mc, o), want, (i, "no colours"))
    same(host(eng, xyz, disp, col, r, nb, mc, o, outs=()), want, (i, "no outputs"))
    same(device(eng, xyz, disp, col, r, nb, mc, o, outs=()), want, (i, "no outputs"))


def test_colours_given_but_not_asked_for_are_ignored(eng):
    xyz, disp, col = layered()
    same(device(eng, xyz, disp, col, 0.02, 8, outs=("keep", "points")), RR.case_want(7))


# ---- 2. inputs that exercise both branches ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,nb,frac", [(0.02, 8, 0.67), (0.02, 16, 0.44), (0.01, 4, 0.31)])
def test_both_branches_on_the_layered_cloud(eng, r, nb, frac):
    xyz, disp, col = layered()
    want = RR.cells(xyz, disp, col, r, nb, RR.FULL)
    share = want["n_kept"] / int(want["in_range"].sum())
    assert 0.05 < share < 0.95 and abs(share - frac) < 0.006 and int(want["in_range"].sum()) == 13576
    both(eng, xyz, disp, col, r, nb, RR.FULL, want=want, what=(r, nb))
    sat = RR.cells(xyz, disp, col, r, nb)
    assert np.array_equal(sat["keep"], want["keep"])
    both(eng, xyz, disp, col, r, nb, want=sat, what=(r, nb, "saturating"))


# ---- 3. geometry in closed form -----------------------------------------------------------------------------------------------------
def test_pairs_straddling_every_face_edge_and_corner(eng):
    for origin in ((0.0, 0.0, 0.0), (0.3, -1.7, 2.2)):
        xyz, dirs = RR.face_pairs(0.25, origin)
        want = both(eng, xyz, None, None, 0.25, 1, 3, origin, what="faces")
        assert want["counts"].tolist() == [1] * 52 and want["n_kept"] == 52 and len(dirs) == 26


def test_the_exact_lattice(eng):
    xyz, nbd = RR.lattice(9, 0.25, (-1.0, 0.5, 2.0))
    want = both(eng, xyz, None, None, 0.25, 6, RR.FULL, what="lattice")
    assert np.array_equal(want["counts"], 6 - nbd) and sorted(set(want["counts"].tolist())) == [3, 4, 5, 6] and want["n_kept"] == 7 ** 3
    xyz, _ = RR.lattice(9, 0.75)
    want = both(eng, xyz, None, None, 0.25, 1, what="lattice at 3 r")
    assert want["counts"].max() == 0 and want["n_kept"] == 0


@pytest.mark.parametrize("mc", [8, RR.FULL])
def test_4096_identical_points_in_one_cell(eng, mc):
    xyz = np.tile(np.array([[0.3, -0.2, 1.7]], np.float32), (4096, 1))
    col = np.arange(4096 * 3, dtype=np.uint32).astype(np.uint8).reshape(-1, 3)
    want = dict(keep=np.ones(4096, np.uint8), counts=np.full(4096, min(4095, mc), np.uint32), points=xyz, colors=col,
                index=np.arange(4096, dtype=np.uint32), n_kept=4096, n_out_of_range=0)
    both(eng, xyz, None, col, 0.05, 8, mc, want=want, what=("one cell", mc))


def test_every_point_invalid(eng):
    xyz, disp, col = layered()
    n = xyz.shape[0]
    assert both(eng, xyz, np.zeros(n, np.float32), col, 0.02, 1, what="disp 0")["n_kept"] == 0
    bad = np.array(xyz)
    bad[np.arange(n), np.arange(n) % 3] = np.nan
    assert both(eng, bad, None, col, 0.02, 1, what="nan")["n_kept"] == 0
    w = both(eng, np.full((n, 3), 3e38, np.float32), None, None, 1.0, 1, what="all out of range")
    assert w["n_out_of_range"] == n and w["n_kept"] == 0


def test_negative_coordinates_and_a_nonzero_origin(eng):
    xyz, disp, col = layered()
    neg = -np.abs(np.array(xyz)) - np.float32(0.37)
    w = both(eng, neg, disp, col, 0.02, 8, 12, what="negative")
    assert 0.05 < w["n_kept"] / w["in_range"].sum() < 0.95 and (w["points"] < 0).all()
    w = both(eng, xyz, disp, col, 0.02, 8, 12, (0.013, -2.5, 100.0), what="origin")
    assert np.array_equal(w["counts"], RR.cells(xyz, disp, None, 0.02, 8, 12)["counts"])      # (in range either way: the origin shows nowhere)


def test_out_of_range_points_beside_ordinary_ones(eng):
    """r = 1e-5: the range ends at about 0.68, so the cloud's far side is out of range although its points are finite, and the in-range
    duplicates next to the border count each other only"""
    r = 1.0e-5
    _, v, _ = RR.constants(r)
    edge = np.float32(65536.0) * v
    inside = np.nextafter(edge, np.float32(0))
    xyz = np.array([[inside, 0, 0], [inside, 0, 0], [edge, 0, 0], [edge, 0, 0], [0.1, 0.1, 0.1], [0.1, 0.1, 0.1], [0.1, 0.1, 0.1],
                    [5.0, 0, 0], [0, -edge, 0], [0, np.nextafter(-edge, np.float32(-9)), 0], [0, -edge, 0]], np.float32)
    w = both(eng, xyz, None, None, r, 1, 5, what="border")
    assert w["counts"].tolist() == [1, 1, 0, 0, 2, 2, 2, 0, 1, 0, 1] and w["n_out_of_range"] == 4 and w["n_kept"] == 7
    lx, ld, lc = layered()
    far = np.array(lx)
    far[5::7, 0] = 3.0e5
    far[3::11, 2] = -1.0e30
    w = both(eng, far, ld, lc, 0.02, 8, what="out of range")
    assert w["n_out_of_range"] > 2500 and w["n_kept"] > 500 and not w["keep"][~w["in_range"]].any()


# ---- 4. the two debug bits, determinism ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [TIGHT, SOURCE, TIGHT | SOURCE])
def test_the_debug_bits_give_the_same_bits(bits):
    """... on the shape cases, and on a table at load exactly 1.0: 16 x 16 x 16 points, each in a cell of its own, in 4096 slots"""
    e = Engine(P16)
    own, _ = RR.lattice(16, 0.5)
    plain = [bytes_of(host(e, *RR.case_input(i)[:3], *RR.SHAPE_CASES[i][3:])) for i in range(NCASE)] + [bytes_of(host(e, own, None, None, 0.25, 1))]
    try:
        e.set_option(_lib.SGM_OPT_DEBUG, bits)
        for i in range(NCASE):
            xyz, disp, col = RR.case_input(i)
            r, nb, mc, o = RR.SHAPE_CASES[i][3:]
            g = host(e, xyz, disp, col, r, nb, mc, o)
            same(g, RR.case_want(i), (bits, i))
            assert bytes_of(g) == plain[i]
            same(device(e, xyz, disp, col, r, nb, mc, o), RR.case_want(i), (bits, i, "device"))
        w = both(e, own, None, None, 0.25, 1, what="load 1.0")
        assert w["counts"].max() == 0 and w["in_range"].sum() == 4096
        assert bytes_of(host(e, own, None, None, 0.25, 1)) == plain[-1]
        assert both(e, own, None, None, 0.5, 3, RR.FULL, what="tight, with neighbours")["counts"].max() == 6
    finally:
        e.set_option(_lib.SGM_OPT_DEBUG, 0)


def test_five_calls_give_the_same_bytes(eng):
    xyz, disp, col = layered()
    runs = [bytes_of(device(eng, xyz, disp, col, 0.02, 8, RR.FULL)) for _ in range(5)]
    assert all(r == runs[0] for r in runs[1:])
    same(device(eng, xyz, disp, col, 0.02, 8, RR.FULL), RR.cells(xyz, disp, col, 0.02, 8, RR.FULL))


# ---- 5. engine state -----------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_the_engine_did_before():
    e = Engine(P16)
    def run(i, fn):
        xyz, disp, col = RR.case_input(i)
        r, nb, mc, o = RR.SHAPE_CASES[i][3:]
        same(fn(e, xyz, disp, col, r, nb, mc, o), RR.case_want(i), (i, fn.__name__))
    big, small = 8, 5                       # 48 x 320, then 257 points
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
        same(device(e, xyz, disp, col, 0.02, 8), RR.case_want(7))
        st = {n: launches for n, ms, launches in e.stage_times()}
        assert st == {"radius_count": 1, "radius_clear": 1, "radius_insert": 1, "radius_starts": 1, "radius_sort": 1, "radius_query": 1,
                      "radius_compact": 3, "_wall": 0}, st
        same(device(e, xyz, disp, col, 0.02, 8, outs=("keep",)), RR.case_want(7))
        assert dict((n, k) for n, ms, k in e.stage_times())["radius_compact"] == 2
    finally:
        e.set_option(_lib.SGM_OPT_PROFILE, 0)


def test_refusals_leave_the_outputs_untouched_and_the_engine_usable(eng):
    L = _lib.load()
    xyz, disp, col = layered()
    xyz, col = np.array(xyz[:100]), np.array(col[:100])
    n = 100
    keep, cnt = np.full(n, MARK_K, np.uint8), np.full(n, MARK_C, np.uint32)
    pts, rgb, idx = np.full((n, 3), MARK_F, np.float32), np.full((n, 3), MARK_B, np.uint8), np.full(n, MARK_C, np.uint32)
    nk, noor = C.c_int64(-5), C.c_int64(-6)
    org, nan_org = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(0, float("nan"), 0)
    X, Cc = xyz.ctypes.data, col.ctypes.data
    out = (keep.ctypes.data, cnt.ctypes.data, pts.ctypes.data, rgb.ctypes.data, idx.ctypes.data)
    NK, NO = C.byref(nk), C.byref(noor)
    h = eng._h
    bad = [
        (None, X, None, Cc, n, 0.05, org, 1, 1) + out + (NK, NO), (h, None, None, Cc, n, 0.05, org, 1, 1) + out + (NK, NO),
        (h, X, None, Cc, n, 0.05, org, 1, 1) + out + (None, NO), (h, X, None, Cc, -1, 0.05, org, 1, 1) + out + (NK, NO),
        (h, X, None, Cc, n, 0.0, org, 1, 1) + out + (NK, NO), (h, X, None, Cc, n, -1.0, org, 1, 1) + out + (NK, NO),
        (h, X, None, Cc, n, float("nan"), org, 1, 1) + out + (NK, NO), (h, X, None, Cc, n, float("inf"), org, 1, 1) + out + (NK, NO),
        (h, X, None, Cc, n, 1e-45, org, 1, 1) + out + (NK, NO), (h, X, None, Cc, n, 1e-20, org, 1, 1) + out + (NK, NO),
        (h, X, None, Cc, n, 1e20, org, 1, 1) + out + (NK, NO),
        (h, X, None, Cc, n, 0.05, nan_org, 1, 1) + out + (NK, NO), (h, X, None, Cc, n, 0.05, None, 1, 1) + out + (NK, NO),
        (h, X, None, Cc, n, 0.05, org, 0, 1) + out + (NK, NO), (h, X, None, Cc, n, 0.05, org, -3, 1) + out + (NK, NO),
        (h, X, None, Cc, n, 0.05, org, 4, 3) + out + (NK, NO), (h, X, None, None, n, 0.05, org, 1, 1) + out + (NK, NO),
    ]
    for fn in (L.sgm_radius_outlier, L.sgm_radius_outlier_device):
        for args in bad:
            assert fn(*args) == -1, args                                   # SGM_ERR_INVALID_ARG
            assert b"sgm_radius_outlier" in L.sgm_last_error()
        assert fn(h, X, None, Cc, 1 << 24, 0.05, org, 1, 1, *out, NK, NO) == -4     # SGM_ERR_UNSUPPORTED: before anything is read
        assert b"2^24" in L.sgm_last_error()
    assert (keep == MARK_K).all() and (cnt == MARK_C).all() and (pts == MARK_F).all() and (rgb == MARK_B).all() and (idx == MARK_C).all()
    assert (nk.value, noor.value) == (-5, -6)
    # n = 0 succeeds with nothing kept and nothing written
    for fn in (L.sgm_radius_outlier, L.sgm_radius_outlier_device):
        nk.value, noor.value = -5, -6
        assert fn(h, X, None, None, 0, 0.05, org, 1, 1, out[0], out[1], out[2], None, out[4], NK, NO) == 0 and (nk.value, noor.value) == (0, 0)
        assert fn(h, X, None, None, 0, 0.05, org, 1, 1, None, None, None, None, None, NK, None) == 0
    assert (keep == MARK_K).all() and (cnt == MARK_C).all() and (pts == MARK_F).all() and (idx == MARK_C).all()
    a, b, c = layered()
    both(eng, a, b, c, 0.02, 8, want=RR.case_want(7), what="after the refusals")


def test_the_other_cloud_calls_are_unchanged_after_a_radius_call():
    e = Engine(P16)
    xyz, disp, col = VR.layered_cloud(97, 331, 9)
    mask = ~np.isnan(xyz[:, :, 0]) & ~np.isinf(xyz[:, :, 0]) & (disp > 0)
    lst = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)

    def radius():
        g = host(e, *lst, 0.02, 8)
        assert 0 < g["n_kept"] < mask.sum()
        return bytes_of(g)
    first = radius()
    p, c = e.compact_points_host(xyz, disp, col)
    assert np.array_equal(p.view(np.uint32), xyz[mask].view(np.uint32)) and np.array_equal(c, col[mask])
    assert radius() == first
    w = VR.voxel_downsample(*lst, 0.05, (0, 0, 0), 2)
    p, c, k, noor = e.voxel_downsample_host(*lst, 0.05, (0, 0, 0), 2, return_counts=True)
    assert np.array_equal(p.view(np.uint32), w["points"].view(np.uint32)) and np.array_equal(c, w["colors"]) and np.array_equal(k, w["counts"])
    assert radius() == first
    w = MR.mesh_grid(xyz, disp, col, 1.0)
    v, c, f = e.mesh_grid_host(xyz, disp, col, 1.0)
    assert np.array_equal(v.view(np.uint32), w["vertices"].view(np.uint32)) and np.array_equal(c, w["colors"]) and np.array_equal(f, w["faces"])
    assert radius() == first
    nrm = e.normals_grid_host(xyz, disp, 1.0, True)
    assert np.array_equal(nrm.view(np.uint32), NR.normal_image(xyz, disp, 1.0, 1).view(np.uint32))
    assert radius() == first


# ---- 6. the Python surface -------------------------------------------------------------------------------------------------------------
def test_remove_radius_outlier_on_numpy_input():
    xyz, disp, col = VR.layered_cloud(48, 320, 31)
    lst = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)
    want = RR.cells(*lst, 0.02, 8)
    assert 0.05 < want["n_kept"] / want["in_range"].sum() < 0.95
    p, c = sgm.remove_radius_outlier(xyz, col, disp, 8, 0.02)
    assert p.dtype == np.float32 and c.dtype == np.uint8
    assert np.array_equal(p.view(np.uint32), want["points"].view(np.uint32)) and np.array_equal(c, want["colors"])
    p, c, mask, cnt, idx = sgm.remove_radius_outlier(xyz, col, disp, 8, 0.02, return_mask=True, return_counts=True, return_index=True)
    assert mask.shape == cnt.shape == disp.shape and mask.dtype == np.uint8 and cnt.dtype == np.uint32 and idx.dtype == np.uint32
    assert np.array_equal(mask.reshape(-1), want["keep"]) and np.array_equal(cnt.reshape(-1), want["counts"]) and np.array_equal(idx, want["index"])
    assert np.array_equal(p.view(np.uint32), xyz.reshape(-1, 3)[idx].view(np.uint32))
    p, c, cnt = sgm.remove_radius_outlier(xyz, None, disp, 8, 0.02, max_count=50, return_counts=True)
    assert c is None and np.array_equal(cnt.reshape(-1), RR.cells(lst[0], lst[1], None, 0.02, 8, 50)["counts"])
    # the mask as the confidence of the other cloud functions
    vp, vc = sgm.valid_points(xyz, col, disp, confidence=mask, min_confidence=1)
    sel = (mask.reshape(-1) == 1) & ~np.isnan(lst[0][:, 0])
    assert np.array_equal(vp.view(np.uint32), want["points"].view(np.uint32)) and np.array_equal(vc, want["colors"]) and sel.sum() == want["n_kept"]
    mv, mc_, mf = sgm.triangulate_points(xyz, col, disp, 1.0, confidence=mask, min_confidence=1)
    w = MR.mesh_grid(xyz, np.where(mask >= 1, disp, np.float32(0)), col, 1.0)
    full = MR.mesh_grid(xyz, disp, col, 1.0)
    assert np.array_equal(mv.view(np.uint32), w["vertices"].view(np.uint32)) and np.array_equal(mf, w["faces"]) and np.array_equal(mc_, w["colors"])
    assert 0 < w["n_faces"] < full["n_faces"]
    # a list without a disparity map, another origin, a confidence map
    w2 = RR.cells(lst[0], None, lst[2], 0.03, 5, 9, (0.5, 0.5, 0.5))
    p, c, m2, k2 = sgm.remove_radius_outlier(lst[0], lst[2], None, 5, 0.03, origin=(0.5, 0.5, 0.5), max_count=9, return_mask=True, return_counts=True)
    assert m2.shape == k2.shape == (lst[0].shape[0],) and np.array_equal(m2, w2["keep"]) and np.array_equal(k2, w2["counts"])
    assert np.array_equal(p.view(np.uint32), w2["points"].view(np.uint32)) and np.array_equal(c, w2["colors"])
    conf = np.random.default_rng(3).integers(0, 101, size=disp.shape).astype(np.uint8)
    w3 = RR.cells(lst[0], np.where(conf >= 40, disp, np.float32(0)).reshape(-1), lst[2], 0.02, 4)
    p, c = sgm.remove_radius_outlier(xyz, col, disp, 4, 0.02, confidence=conf, min_confidence=40)
    assert 0 < w3["n_kept"] and np.array_equal(p.view(np.uint32), w3["points"].view(np.uint32)) and np.array_equal(c, w3["colors"])
    out = sgm.remove_radius_outlier(np.zeros((0, 3), np.float32), None, None, 4, 0.1, return_mask=True)
    assert out[0].shape == (0, 3) and out[1] is None and out[2].shape == (0,)


def test_a_270_x_480_frame_from_the_pipeline():
    """270 x 480 through sgm_pipeline_device, then the device entry on the resident XYZ image.  The radius is 2.5 times the median
    spacing of horizontal neighbours; nb_points is the 40th percentile of the REFERENCE's full counts, so that both branches run."""
    import torch
    H, W, D = 270, 480, 64
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
    xyz, disp, col = dx.cpu().numpy(), df.cpu().numpy(), rgb.cpu().numpy()
    ok = np.isfinite(xyz).all(axis=2) & (disp > 0)
    assert ok.mean() > 0.3
    with np.errstate(all="ignore"):
        step = np.abs(xyz[:, 1:, 0] - xyz[:, :-1, 0])[ok[:, 1:] & ok[:, :-1]]
    r = float(np.float32(2.5 * np.median(step)))
    lst = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)
    full = RR.cells(*lst, r, 1, RR.FULL)
    nb = max(1, int(np.percentile(full["full"][full["in_range"]], 40)))
    keep = (full["full"] >= nb).astype(np.uint8)
    assert 0.05 < keep.sum() / full["in_range"].sum() < 0.95 and nb >= 2
    idx = np.nonzero(keep)[0]
    want = dict(keep=keep, counts=np.minimum(full["full"], nb + 3).astype(np.uint32), points=lst[0][idx], colors=lst[2][idx],
                index=idx.astype(np.uint32), n_kept=int(idx.size), n_out_of_range=full["n_out_of_range"])
    n = H * W
    t = dict(keep=torch.full((n,), MARK_K, dtype=torch.uint8, device="cuda"), counts=torch.full((n,), -1, dtype=torch.int32, device="cuda"),
             points=torch.full((n, 3), float(MARK_F), dtype=torch.float32, device="cuda"),
             colors=torch.full((n, 3), MARK_B, dtype=torch.uint8, device="cuda"),
             index=torch.from_numpy(np.full(n, MARK_C, np.uint32).view(np.int32)).cuda())
    torch.cuda.synchronize()
    nk, noor = e.radius_outlier_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), n, r, nb, nb + 3, (0, 0, 0),
                                       *(t[k].data_ptr() for k in ALL))
    g = {k: x.cpu().numpy() for k, x in t.items()}
    g["counts"], g["index"] = g["counts"].view(np.uint32), g["index"].view(np.uint32)
    same(dict(g, n=n, n_kept=nk, n_out_of_range=noor), want, "pipeline frame")
    assert np.array_equal(dx.cpu().numpy(), xyz, equal_nan=True)
    # the package function on the same frame
    p, c, mask = sgm.remove_radius_outlier(xyz, col, disp, nb, r, return_mask=True)
    assert np.array_equal(mask.reshape(-1), keep) and np.array_equal(p.view(np.uint32), want["points"].view(np.uint32)) and np.array_equal(c, want["colors"])


# ---- 7. full size ----------------------------------------------------------------------------------------------------------------------
def test_a_full_size_planar_lattice():
    """2160 x 4096 points at spacing 0.25 in the plane Z = 2, r = 0.375: the neighbours of a point are the other points of its 3 x 3
    box (0.25 and 0.3536 away; the next ring is 0.5 away), every coordinate, difference and square is exact.  8.8 M points in the
    largest table the call can need (2^25 slots)."""
    import torch
    H, W = 2160, 4096
    n = H * W
    e = Engine(P16)
    y, x = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    dx = torch.stack([x * 0.25 - 300.0, y * 0.25 - 100.0, torch.full_like(x, 2.0)], dim=2).reshape(n, 3).contiguous()
    edge_y, edge_x = ((y == 0) | (y == H - 1)).reshape(n), ((x == 0) | (x == W - 1)).reshape(n)
    want = torch.full((n,), 8, dtype=torch.int32, device="cuda")
    want[edge_y | edge_x] = 5
    want[edge_y & edge_x] = 3
    del x, y
    keep = torch.full((n,), MARK_K, dtype=torch.uint8, device="cuda")
    cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    pts = torch.full((n, 3), float(MARK_F), dtype=torch.float32, device="cuda")
    before = dx.clone()
    torch.cuda.synchronize()
    nk, noor = e.radius_outlier_device(dx.data_ptr(), None, None, n, 0.375, 8, RR.FULL, (0, 0, 0), keep.data_ptr(), cnt.data_ptr(),
                                       pts.data_ptr(), None, idx.data_ptr())
    inner = (H - 2) * (W - 2)
    assert (nk, noor) == (inner, 0)
    assert bool((cnt == want).all()) and bool((keep == (want == 8).to(torch.uint8)).all())
    src = torch.nonzero(want == 8).reshape(-1).to(torch.int32)
    assert bool((idx[:inner] == src).all()) and bool((idx[inner:] == -1).all())
    assert bool((pts[:inner] == dx[src.long()]).all()) and bool((pts[inner:] == float(MARK_F)).all()) and bool((dx == before).all())
    nk5, _ = e.radius_outlier_device(dx.data_ptr(), None, None, n, 0.375, 5, 5, (0, 0, 0), keep.data_ptr(), cnt.data_ptr())
    assert nk5 == n - 4 and bool((cnt == torch.clamp(want, max=5)).all()) and bool((keep == (want >= 5).to(torch.uint8)).all())


# ---- 8. guarded buffers -------------------------------------------------------------------------------------------------------------------
def test_the_cases_with_every_buffer_guarded():
    """(the same cases ran in the plain mode above)"""
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "radius_guard_child.py")], capture_output=True, text=True, env=env,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"RADIUS_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) >= 14, tail
