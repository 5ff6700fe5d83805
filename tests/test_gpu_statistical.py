"""Statistical outlier removal on the device (needs an MI355X): sgm_statistical_outlier, sgm_statistical_outlier_device,
Engine.statistical_outlier_host / _device, sgm.remove_statistical_outlier.

Yardstick: tests/statistical_ref.py -- the definition of include/sgm_hip_statistical.h in numpy, over all pairs or over 27 cells
-- bit for bit: keep, the means (as uint32), points, colours, index, n_kept and the eight statistics, through both entries.  Every
output is pre-filled with a marker, so rows past n_kept are seen untouched, and every input is checked unmodified."""
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
import statistical_ref as SR
import voxel_ref as VR
import stereo_reconstruction_cv_amd as sgm
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = dict(numDisparities=16)
NCASE = len(SR.SHAPE_CASES)
MARK_F, MARK_B, MARK_C, MARK_K, MARK_S = np.float32(-77.25), 177, 0xDEADBEEF, 99, 0xABCDEF0123456789
ALL = ("keep", "mean", "points", "colors", "index", "stats")


@pytest.fixture(scope="module")
def eng():
    return Engine(P16)


@functools.lru_cache(maxsize=None)
def layered():
    """the 48 x 320 layered cloud as lists, shared and read-only"""
    return SR.layered_lists(48, 320, 704)


def host(e, xyz, disp, col, k, ratio, r, o=(0, 0, 0), outs=ALL):
    """the host entry called on marked outputs: a dict of whole arrays (None where not asked for) and n_kept"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    before = [xyz.copy(), None if disp is None else np.array(disp), None if col is None else np.array(col)]
    m = max(n, 1)
    g = dict(keep=np.full(m, MARK_K, np.uint8) if "keep" in outs else None,
             mean=np.full(m, MARK_F, np.float32) if "mean" in outs else None,
             points=np.full((m, 3), MARK_F, np.float32) if "points" in outs else None,
             colors=np.full((m, 3), MARK_B, np.uint8) if "colors" in outs and col is not None else None,
             index=np.full(m, MARK_C, np.uint32) if "index" in outs else None,
             stats=np.full(8, MARK_S, np.uint64) if "stats" in outs else None)
    org = np.asarray(o, np.float32)
    nk = C.c_int64(-5)
    at = lambda a: None if a is None else a.ctypes.data
    rc = _lib.load().sgm_statistical_outlier(e._h, xyz.ctypes.data, at(disp), at(col), n, int(k), float(ratio), float(r), org.ctypes.data,
                                             at(g["keep"]), at(g["mean"]), at(g["points"]), at(g["colors"]), at(g["index"]), C.byref(nk),
                                             at(g["stats"]))
    assert rc == 0, _lib.last_error()
    assert np.array_equal(xyz, before[0], equal_nan=True) and (disp is None or np.array_equal(disp, before[1], equal_nan=True))
    assert col is None or np.array_equal(col, before[2])
    return dict(g, n=n, n_kept=nk.value)


def device(e, xyz, disp, col, k, ratio, r, o=(0, 0, 0), outs=ALL):
    """the same through the device entry, every array a tensor of its own"""
    import torch
    dev = torch.device("cuda", e.device)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    dx, dd, dc = up(xyz), up(disp), up(col)
    m = max(n, 1)
    t = dict(keep=torch.full((m,), MARK_K, dtype=torch.uint8, device=dev) if "keep" in outs else None,
             mean=torch.full((m,), float(MARK_F), dtype=torch.float32, device=dev) if "mean" in outs else None,
             points=torch.full((m, 3), float(MARK_F), dtype=torch.float32, device=dev) if "points" in outs else None,
             colors=torch.full((m, 3), MARK_B, dtype=torch.uint8, device=dev) if "colors" in outs and col is not None else None,
             index=torch.from_numpy(np.full(m, MARK_C, np.uint32).view(np.int32)).to(dev) if "index" in outs else None)
    p = lambda x: None if x is None else x.data_ptr()
    torch.cuda.synchronize()
    nk, stats = e.statistical_outlier_device(p(dx), p(dd), p(dc), n, k, ratio, r, o, p(t["keep"]), p(t["mean"]), p(t["points"]),
                                             p(t["colors"]), p(t["index"]))
    e.synchronize()
    assert np.array_equal(dx.cpu().numpy(), xyz, equal_nan=True) and (disp is None or np.array_equal(dd.cpu().numpy(), disp, equal_nan=True))
    assert col is None or np.array_equal(dc.cpu().numpy(), col)
    g = {k_: None if x is None else x.cpu().numpy() for k_, x in t.items()}
    g["index"] = None if g["index"] is None else g["index"].view(np.uint32)
    return dict(g, stats=stats, n=n, n_kept=nk)


def same(got, want, what=""):
    """bit for bit against a reference result, and the rows behind n_kept untouched"""
    n, m = got["n"], want["n_kept"]
    assert got["n_kept"] == m, (what, got["n_kept"], m)
    if got["stats"] is not None:
        assert got["stats"].dtype == np.uint64 and got["stats"].tolist() == want["stats"].tolist(), (what, got["stats"], want["stats"])
    if got["keep"] is not None:
        assert got["keep"].dtype == np.uint8 and np.array_equal(got["keep"][:n], want["keep"]), (what, "keep")
    if got["mean"] is not None:
        bad = np.nonzero(got["mean"][:n].view(np.uint32) != want["mean"].view(np.uint32))[0]
        assert got["mean"].dtype == np.float32 and bad.size == 0, (what, "mean", bad[:5], got["mean"][bad[:5]], want["mean"][bad[:5]])
    if got["points"] is not None:
        assert np.array_equal(got["points"][:m].view(np.uint32), want["points"].view(np.uint32)) and (got["points"][m:] == MARK_F).all(), what
    if got["colors"] is not None:
        assert np.array_equal(got["colors"][:m], want["colors"]) and (got["colors"][m:] == MARK_B).all(), what
    if got["index"] is not None:
        assert np.array_equal(got["index"][:m], want["index"]) and (got["index"][m:] == MARK_C).all(), what


def both(e, xyz, disp, col, k, ratio, r, o=(0, 0, 0), want=None, what=""):
    if want is None:
        want = SR.cells(np.asarray(xyz, np.float32).reshape(-1, 3), disp, col, k, ratio, r, o)
    same(host(e, xyz, disp, col, k, ratio, r, o), want, (what, "host"))
    same(device(e, xyz, disp, col, k, ratio, r, o), want, (what, "device"))
    return want


def bytes_of(g):
    return [None if g[k] is None else g[k].tobytes() for k in ALL] + [g["n_kept"]]


def stats(w):
    return dict(zip(SR.STATS, (int(x) for x in w["stats"])))


# ---- 1. shapes, through both entries, with and without disp, colours and each optional output -------------------------------------
@pytest.mark.parametrize("i", range(NCASE))
def test_shapes_through_both_entries(eng, i):
    kind, a, b, k, ratio, r, o = SR.SHAPE_CASES[i]
    xyz, disp, col = SR.case_input(i)
    for with_disp in ((True, False) if disp is not None else (False,)):
        want = SR.case_want(i, with_disp)
        for fn in (host, device):
            same(fn(eng, xyz, disp if with_disp else None, col, k, ratio, r, o), want, (i, fn.__name__, with_disp))
    want = SR.case_want(i)
    for out, fn in zip(ALL, (host, device, host, device, host, device)):           # each output alone, and none at all
        same(fn(eng, xyz, disp, col, k, ratio, r, o, outs=(out,)), want, (i, "only", out))
    same(device(eng, xyz, disp, None, k, ratio, r, o), want, (i, "no colours"))
    same(host(eng, xyz, disp, col, k, ratio, r, o, outs=()), want, (i, "no outputs"))
    same(device(eng, xyz, disp, col, k, ratio, r, o, outs=()), want, (i, "no outputs"))


def test_colours_given_but_not_asked_for_are_ignored(eng):
    xyz, disp, col = layered()
    same(device(eng, xyz, disp, col, 8, 1.0, 0.02, outs=("keep", "points")), SR.case_want(7))


# ---- 2. k and the edges of the capacity classes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 8, 9, 16, 17, 32, 33, 64])
def test_every_k_at_the_edges_of_the_list_capacities(eng, k):
    """the lists of k_stat_query hold 8, 16, 32 or 64 values.  On the 24 x 130 cloud r = 0.05 gives a point up to 140 neighbours;
    k = 1 and 4 take a smaller and k = 64 a larger radius, so that there are dense and sparse points at every k"""
    r = {1: 0.012, 4: 0.03, 64: 0.1}.get(k, 0.05)
    xyz, disp, col = SR.layered_lists(24, 130, 724)
    want = SR.layered_want(24, 130, 724, k, 1.0, r)
    s = stats(want)
    assert s["dense"] > 200 and s["sparse"] > 200 and 0 < want["n_kept"] < s["dense"], s
    both(eng, xyz, disp, col, k, 1.0, r, want=want, what=k)


def test_exactly_64_and_63_neighbours_at_k_64(eng):
    """65 copies of one point (64 neighbours each: dense, mean 0), 64 copies of another (63 each: sparse), and a point with 64
    neighbours at 64 different distances, whose own neighbours on the line have fewer"""
    a = np.tile(np.array([[500.5, 0.5, 0.5]], np.float32), (65, 1))
    b = np.tile(np.array([[-503.0, 1.0, 0.25]], np.float32), (64, 1))
    ring = np.zeros((65, 3), np.float32)
    ring[:, 0] = 10.0
    ring[1:, 1] = (np.arange(64, dtype=np.float32) + 1) * np.float32(0.3) * np.where(np.arange(64) % 2, -1, 1).astype(np.float32)
    xyz = np.concatenate([a, b, ring])
    want = both(eng, xyz, None, None, 64, 1.0, 20.0, what="64 / 63")
    assert want["dense"][:65].all() and not want["dense"][65:129].any() and want["dense"][129] and not want["dense"][130:].all()
    assert (want["mean"][:65] == 0).all() and (want["mean"][65:129] == -1).all() and want["mean"][129] > 9.0


# ---- 3. the kept-share rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", SR.SHARE_ROWS + [SR.SPARSE_ROW])
def test_the_kept_share_rows(eng, row):
    H, W, seed, r, k, ratio, dense, sparse, kept = row[:9]
    want = SR.layered_want(H, W, seed, k, ratio, r)
    s = stats(want)
    assert (s["dense"], s["sparse"], want["n_kept"]) == (dense, sparse, kept)          # the reference first: a drift shows as such
    if len(row) == 10:
        assert s["T"] == row[9] and 0.05 < kept / s["in_range"] < 0.95
    both(eng, *SR.layered_lists(H, W, seed), k, ratio, r, want=want, what=row)


# ---- 4. geometry in closed form -----------------------------------------------------------------------------------------------------
def test_pairs_straddling_every_face_edge_and_corner(eng):
    for origin in ((0.0, 0.0, 0.0), (0.3, -1.7, 2.2)):
        xyz, dirs = SR.face_pairs(0.25, origin)
        want = both(eng, xyz, None, None, 1, 1.0, 0.25, origin, what="faces")
        assert want["dense"].all() and len(dirs) == 26 and (want["mean"] > 0).all() and (want["mean"] < 0.25).all()


def test_the_exact_lattice(eng):
    """9^3 points at spacing 0.25, r = 0.375: 6 neighbours at 0.25 and 12 at 0.3536 for an interior point, so with k = 6 its mean
    is exactly 0.25; every point has at least 3 + 3 neighbours, so all are dense"""
    xyz, nbd = SR.lattice(9, 0.25, (-1.0, 0.5, 2.0))
    want = both(eng, xyz, None, None, 6, 1.0, 0.375, what="lattice")
    assert want["dense"].all() and (want["mean"][nbd == 0] == 0.25).all() and (nbd == 0).sum() == 7 ** 3
    assert (want["mean"][nbd > 0] > 0.25).all() and want["keep"][nbd == 0].all()


def test_4096_identical_points_in_one_cell(eng):
    xyz = np.tile(np.array([[0.3, -0.2, 1.7]], np.float32), (4096, 1))
    col = np.arange(4096 * 3, dtype=np.uint32).astype(np.uint8).reshape(-1, 3)
    want = dict(keep=np.ones(4096, np.uint8), mean=np.zeros(4096, np.float32), points=xyz, colors=col, index=np.arange(4096, dtype=np.uint32),
                n_kept=4096, stats=np.array([4096, 0, 4096, 0, 0, 0, 0, 0], np.uint64))
    both(eng, xyz, None, col, 64, 1.0, 0.05, want=want, what="one cell")


def test_distances_whose_squares_are_denormal(eng):
    """two points 2^-70 apart among ordinary ones: d2 = 2^-140 is a denormal binary32 number, its root 2^-70 is not"""
    xyz, _ = SR.random_list(300, 77, 0.5)
    xyz = np.array(xyz)
    xyz[10] = (0.0, 0.125, -0.25)
    xyz[200] = (np.float32(2.0 ** -70), 0.125, -0.25)
    want = both(eng, xyz, None, None, 1, 1.0, 0.1, what="denormal")
    assert want["mean"][10] == want["mean"][200] == np.float32(2.0 ** -70) and want["q"][10] == 0 and want["keep"][10] == 1
    want = both(eng, xyz, None, None, 2, 1.0, 0.1, what="denormal, k = 2")
    assert want["dense"][10] and want["mean"][10] > 1e-3


def test_every_point_invalid_out_of_range_or_sparse(eng):
    xyz, disp, col = layered()
    n = xyz.shape[0]
    w = both(eng, xyz, np.zeros(n, np.float32), col, 1, 1.0, 0.02, what="disp 0")
    assert w["n_kept"] == 0 and w["stats"].tolist() == [0] * 8 and (w["mean"] == -1).all()
    bad = np.array(xyz)
    bad[np.arange(n), np.arange(n) % 3] = np.nan
    assert both(eng, bad, None, col, 1, 1.0, 0.02, what="nan")["n_kept"] == 0
    w = both(eng, np.full((n, 3), 3e38, np.float32), None, None, 1, 1.0, 1.0, what="all out of range")
    assert w["stats"].tolist() == [0, n, 0, 0, 0, 0, 0, 0] and w["n_kept"] == 0
    w = both(eng, xyz, disp, col, 8, 1.0, 1e-4, what="all sparse")
    assert w["stats"].tolist() == [13576, 0, 0, 13576, 0, 0, 0, 0] and w["n_kept"] == 0 and (w["mean"] == -1).all()


def test_negative_coordinates_and_a_nonzero_origin(eng):
    xyz, disp, col = layered()
    neg = -np.abs(np.array(xyz)) - np.float32(0.37)
    w = both(eng, neg, disp, col, 8, 1.0, 0.02, what="negative")
    assert 0.05 < w["n_kept"] / w["in_range"].sum() < 0.95 and (w["points"] < 0).all()
    w = both(eng, xyz, disp, col, 8, 1.0, 0.02, (0.013, -2.5, 100.0), what="origin")
    assert np.array_equal(w["mean"].view(np.uint32), SR.case_want(7)["mean"].view(np.uint32))     # (in range either way: the origin shows nowhere)


def test_out_of_range_points_beside_ordinary_ones(eng):
    lx, ld, lc = layered()
    far = np.array(lx)
    far[5::7, 0] = 3.0e5
    far[3::11, 2] = -1.0e30
    w = both(eng, far, ld, lc, 8, 1.0, 0.02, what="out of range")
    assert stats(w)["out_of_range"] > 2500 and w["n_kept"] > 500 and not w["keep"][~w["in_range"]].any() and (w["mean"][~w["in_range"]] == -1).all()


# ---- 5. determinism, engine state ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [_lib.SGM_DBG_STAT_WIDE_LIST, _lib.SGM_DBG_RADIUS_TIGHT_TABLE | _lib.SGM_DBG_STAT_WIDE_LIST])
def test_the_debug_bits_give_the_same_bits(bits):
    """the 64-word list at every k, alone and in a table at the tight size: the bytes of the default on the shape cases and at
    the k of every capacity"""
    e = Engine(P16)
    small = SR.layered_lists(24, 130, 724)
    runs = [(SR.case_input(i), SR.SHAPE_CASES[i][3:], SR.case_want(i)) for i in range(NCASE)]
    runs += [(small, (k, 1.0, 0.05, (0, 0, 0)), SR.layered_want(24, 130, 724, k, 1.0, 0.05)) for k in (8, 9, 17, 33)]
    plain = [bytes_of(host(e, *inp, *par)) for inp, par, _ in runs]
    try:
        e.set_option(_lib.SGM_OPT_DEBUG, bits)
        for (inp, par, want), first in zip(runs, plain):
            g = host(e, *inp, *par)
            same(g, want, (bits, par))
            assert bytes_of(g) == first
            same(device(e, *inp, *par), want, (bits, par, "device"))
    finally:
        e.set_option(_lib.SGM_OPT_DEBUG, 0)


def test_five_calls_give_the_same_bytes(eng):
    xyz, disp, col = layered()
    runs = [bytes_of(device(eng, xyz, disp, col, 16, 0.5, 0.04)) for _ in range(5)]
    assert all(r == runs[0] for r in runs[1:])
    same(device(eng, xyz, disp, col, 16, 0.5, 0.04), SR.layered_want(48, 320, 704, 16, 0.5, 0.04))


def test_results_do_not_depend_on_what_the_engine_did_before():
    e = Engine(P16)
    def run(i, fn):
        xyz, disp, col = SR.case_input(i)
        k, ratio, r, o = SR.SHAPE_CASES[i][3:]
        same(fn(e, xyz, disp, col, k, ratio, r, o), SR.case_want(i), (i, fn.__name__))
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
        same(device(e, xyz, disp, col, 8, 1.0, 0.02), SR.case_want(7))
        st = {n: launches for n, ms, launches in e.stage_times()}
        assert st == {"stat_count": 1, "stat_clear": 1, "stat_insert": 1, "stat_starts": 1, "stat_sort": 1, "stat_query": 1,
                      "stat_reduce": 1, "stat_keep": 1, "stat_compact": 3, "_wall": 0}, st
        same(device(e, xyz, disp, col, 8, 1.0, 0.02, outs=("keep",)), SR.case_want(7))
        assert dict((n, k) for n, ms, k in e.stage_times())["stat_compact"] == 2
    finally:
        e.set_option(_lib.SGM_OPT_PROFILE, 0)


def test_refusals_leave_the_outputs_untouched_and_the_engine_usable(eng):
    L = _lib.load()
    xyz, disp, col = layered()
    xyz, col = np.array(xyz[:100]), np.array(col[:100])
    n = 100
    keep, mean = np.full(n, MARK_K, np.uint8), np.full(n, MARK_F, np.float32)
    pts, rgb, idx = np.full((n, 3), MARK_F, np.float32), np.full((n, 3), MARK_B, np.uint8), np.full(n, MARK_C, np.uint32)
    st = np.full(8, MARK_S, np.uint64)
    nk = C.c_int64(-5)
    org, nan_org = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(0, float("nan"), 0)
    X, Cc = xyz.ctypes.data, col.ctypes.data
    out = (keep.ctypes.data, mean.ctypes.data, pts.ctypes.data, rgb.ctypes.data, idx.ctypes.data)
    NK, ST = C.byref(nk), st.ctypes.data
    h = eng._h
    ok = (4, 1.0, 0.05, org)
    bad = [(None, X, None, Cc, n) + ok + out + (NK, ST), (h, None, None, Cc, n) + ok + out + (NK, ST),
           (h, X, None, Cc, n) + ok + out + (None, ST), (h, X, None, Cc, -1) + ok + out + (NK, ST),
           (h, X, None, None, n) + ok + out + (NK, ST)]                                   # out_colors without colours
    bad += [(h, X, None, Cc, n, k, 1.0, 0.05, org) + out + (NK, ST) for k in (0, -3, 65, 1 << 20)]
    bad += [(h, X, None, Cc, n, 4, ratio, 0.05, org) + out + (NK, ST) for ratio in (-1.0, -1e-30, float("nan"), float("inf"))]
    bad += [(h, X, None, Cc, n, 4, 1.0, r, org) + out + (NK, ST) for r in (0.0, -1.0, float("nan"), float("inf"), 1e-45, 1e-20, 1e20)]
    bad += [(h, X, None, Cc, n, 4, 1.0, 0.05, o) + out + (NK, ST) for o in (nan_org, None)]
    for fn in (L.sgm_statistical_outlier, L.sgm_statistical_outlier_device):
        for args in bad:
            assert fn(*args) == -1, args                                   # SGM_ERR_INVALID_ARG
            assert b"sgm_statistical_outlier" in L.sgm_last_error()
        assert fn(h, X, None, Cc, 1 << 24, *ok, *out, NK, ST) == -4     # SGM_ERR_UNSUPPORTED: before anything is read
        assert b"2^24" in L.sgm_last_error()
    assert (keep == MARK_K).all() and (mean == MARK_F).all() and (pts == MARK_F).all() and (rgb == MARK_B).all() and (idx == MARK_C).all()
    assert nk.value == -5 and (st == MARK_S).all()
    # n = 0 succeeds with nothing kept, the statistics zero and nothing else written
    for fn in (L.sgm_statistical_outlier, L.sgm_statistical_outlier_device):
        nk.value = -5
        st[:] = MARK_S
        assert fn(h, X, None, None, 0, *ok, out[0], out[1], out[2], None, out[4], NK, ST) == 0 and nk.value == 0 and st.tolist() == [0] * 8
        assert fn(h, X, None, None, 0, *ok, None, None, None, None, None, NK, None) == 0
    assert (keep == MARK_K).all() and (mean == MARK_F).all() and (pts == MARK_F).all() and (idx == MARK_C).all()
    a, b, c = layered()
    both(eng, a, b, c, 8, 1.0, 0.02, want=SR.case_want(7), what="after the refusals")


def test_the_other_cloud_calls_are_unchanged_with_statistical_calls_between_them():
    e = Engine(P16)
    xyz, disp, col = VR.layered_cloud(97, 331, 9)
    mask = ~np.isnan(xyz[:, :, 0]) & ~np.isinf(xyz[:, :, 0]) & (disp > 0)
    lst = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)

    def statistical():
        g = host(e, *lst, 8, 1.0, 0.03)
        assert 0 < g["n_kept"] < mask.sum()
        return bytes_of(g)
    first = statistical()
    w = RR.cells(*lst, 0.02, 8, 12)
    p, c, keep, cnt, idx, noor = e.radius_outlier_host(*lst, 0.02, 8, 12, return_counts=True, return_index=True)
    assert np.array_equal(keep, w["keep"]) and np.array_equal(cnt, w["counts"]) and np.array_equal(idx, w["index"]) and noor == w["n_out_of_range"]
    assert np.array_equal(p.view(np.uint32), w["points"].view(np.uint32)) and np.array_equal(c, w["colors"])
    assert statistical() == first
    p, c = e.compact_points_host(xyz, disp, col)
    assert np.array_equal(p.view(np.uint32), xyz[mask].view(np.uint32)) and np.array_equal(c, col[mask])
    assert statistical() == first
    w = VR.voxel_downsample(*lst, 0.05, (0, 0, 0), 2)
    p, c, k, noor = e.voxel_downsample_host(*lst, 0.05, (0, 0, 0), 2, return_counts=True)
    assert np.array_equal(p.view(np.uint32), w["points"].view(np.uint32)) and np.array_equal(c, w["colors"]) and np.array_equal(k, w["counts"])
    assert statistical() == first
    w = MR.mesh_grid(xyz, disp, col, 1.0)
    v, c, f = e.mesh_grid_host(xyz, disp, col, 1.0)
    assert np.array_equal(v.view(np.uint32), w["vertices"].view(np.uint32)) and np.array_equal(c, w["colors"]) and np.array_equal(f, w["faces"])
    assert statistical() == first
    nrm = e.normals_grid_host(xyz, disp, 1.0, True)
    assert np.array_equal(nrm.view(np.uint32), NR.normal_image(xyz, disp, 1.0, 1).view(np.uint32))
    assert statistical() == first
    same(host(e, *lst, 8, 1.0, 0.03), SR.cells(*lst, 8, 1.0, 0.03), "97 x 331")


# ---- 6. the Python surface -------------------------------------------------------------------------------------------------------------
def test_remove_statistical_outlier_on_numpy_input():
    xyz, disp, col = VR.layered_cloud(48, 320, 31)
    lst = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)
    want = SR.cells(*lst, 8, 1.0, 0.03)
    assert 0.05 < want["n_kept"] / want["in_range"].sum() < 0.95
    p, c = sgm.remove_statistical_outlier(xyz, col, disp, 8, 1.0, 0.03)
    assert p.dtype == np.float32 and c.dtype == np.uint8
    assert np.array_equal(p.view(np.uint32), want["points"].view(np.uint32)) and np.array_equal(c, want["colors"])
    p, c, mask, dist, idx, st = sgm.remove_statistical_outlier(xyz, col, disp, 8, 1.0, 0.03, return_mask=True, return_distances=True,
                                                               return_index=True, return_stats=True)
    assert mask.shape == dist.shape == disp.shape and mask.dtype == np.uint8 and dist.dtype == np.float32 and idx.dtype == np.uint32
    assert np.array_equal(mask.reshape(-1), want["keep"]) and np.array_equal(dist.reshape(-1).view(np.uint32), want["mean"].view(np.uint32))
    assert np.array_equal(idx, want["index"]) and st == stats(want)
    assert np.array_equal(p.view(np.uint32), xyz.reshape(-1, 3)[idx].view(np.uint32))
    # the mask as the confidence of the other cloud functions
    vp, vc = sgm.valid_points(xyz, col, disp, confidence=mask, min_confidence=1)
    assert np.array_equal(vp.view(np.uint32), want["points"].view(np.uint32)) and np.array_equal(vc, want["colors"])
    mv, mc_, mf = sgm.triangulate_points(xyz, col, disp, 1.0, confidence=mask, min_confidence=1)
    w = MR.mesh_grid(xyz, np.where(mask >= 1, disp, np.float32(0)), col, 1.0)
    full = MR.mesh_grid(xyz, disp, col, 1.0)
    assert np.array_equal(mv.view(np.uint32), w["vertices"].view(np.uint32)) and np.array_equal(mf, w["faces"]) and np.array_equal(mc_, w["colors"])
    assert 0 < w["n_faces"] < full["n_faces"]
    # a list without a disparity map, another origin, a confidence map
    w2 = SR.cells(lst[0], None, lst[2], 5, 0.5, 0.03, (0.5, 0.5, 0.5))
    p, c, m2, d2 = sgm.remove_statistical_outlier(lst[0], lst[2], None, 5, 0.5, 0.03, origin=(0.5, 0.5, 0.5), return_mask=True, return_distances=True)
    assert m2.shape == d2.shape == (lst[0].shape[0],) and np.array_equal(m2, w2["keep"]) and np.array_equal(d2.view(np.uint32), w2["mean"].view(np.uint32))
    assert np.array_equal(p.view(np.uint32), w2["points"].view(np.uint32)) and np.array_equal(c, w2["colors"])
    conf = np.random.default_rng(3).integers(0, 101, size=disp.shape).astype(np.uint8)
    w3 = SR.cells(lst[0], np.where(conf >= 40, disp, np.float32(0)).reshape(-1), lst[2], 4, 1.0, 0.03)
    p, c = sgm.remove_statistical_outlier(xyz, col, disp, 4, 1.0, 0.03, confidence=conf, min_confidence=40)
    assert 0 < w3["n_kept"] and np.array_equal(p.view(np.uint32), w3["points"].view(np.uint32)) and np.array_equal(c, w3["colors"])
    out = sgm.remove_statistical_outlier(np.zeros((0, 3), np.float32), None, None, 4, 1.0, 0.1, return_mask=True)
    assert out[0].shape == (0, 3) and out[1] is None and out[2].shape == (0,)


def test_a_270_x_480_frame_from_the_pipeline():
    """270 x 480 through sgm_pipeline_device, then the device entry on the resident XYZ image.  max_radius is the first of 3.5, 6
    and 10 times the median spacing of horizontal neighbours at which the REFERENCE radius count has a median of at least 2 k."""
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
    lst = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)
    for mult in (3.5, 6.0, 10.0):
        r = float(np.float32(mult * np.median(step)))
        full = RR.cells(*lst, r, 1, RR.FULL)
        if np.median(full["full"][full["in_range"]]) >= 16:
            break
    want = SR.cells(*lst, 8, 1.0, r)
    s = stats(want)
    assert s["dense"] > 0.3 * s["in_range"] and 0 < want["n_kept"] < s["dense"], s
    n = H * W
    t = dict(keep=torch.full((n,), MARK_K, dtype=torch.uint8, device="cuda"),
             mean=torch.full((n,), float(MARK_F), dtype=torch.float32, device="cuda"),
             points=torch.full((n, 3), float(MARK_F), dtype=torch.float32, device="cuda"),
             colors=torch.full((n, 3), MARK_B, dtype=torch.uint8, device="cuda"),
             index=torch.from_numpy(np.full(n, MARK_C, np.uint32).view(np.int32)).cuda())
    torch.cuda.synchronize()
    nk, st = e.statistical_outlier_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), n, 8, 1.0, r, (0, 0, 0),
                                          *(t[k].data_ptr() for k in ALL[:5]))
    g = {k: x.cpu().numpy() for k, x in t.items()}
    g["index"] = g["index"].view(np.uint32)
    same(dict(g, stats=st, n=n, n_kept=nk), want, "pipeline frame")
    assert np.array_equal(dx.cpu().numpy(), xyz, equal_nan=True)
    # the package function on the same frame
    p, c, mask = sgm.remove_statistical_outlier(xyz, col, disp, 8, 1.0, r, return_mask=True)
    assert np.array_equal(mask.reshape(-1), want["keep"]) and np.array_equal(p.view(np.uint32), want["points"].view(np.uint32)) and np.array_equal(c, want["colors"])


# ---- 7. full size ----------------------------------------------------------------------------------------------------------------------
def test_a_full_size_planar_lattice():
    """2160 x 4096 points at spacing 0.25 in the plane Z = 2, r = 0.375, k = 8: the neighbours of a point are the other points of
    its 3 x 3 box, four 0.25 and four 0.3536 away; interior points have 8, edge points 5 and corner points 3, so the interior is
    dense and the rim sparse.  Every coordinate, difference and square is exact and all dense points share one multiset, hence one
    mean and one q: var is exactly 0 and T = q.  8.8 M points in the largest table the call can need (2^25 slots)."""
    import torch
    H, W = 2160, 4096
    n = H * W
    e = Engine(P16)
    y, x = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    dx = torch.stack([x * 0.25 - 300.0, y * 0.25 - 100.0, torch.full_like(x, 2.0)], dim=2).reshape(n, 3).contiguous()
    inner = ((y > 0) & (y < H - 1) & (x > 0) & (x < W - 1)).reshape(n)
    del x, y
    s1, s2 = np.float32(0.25), np.sqrt(np.float32(0.125))
    acc = s1
    for s in (s1, s1, s1, s2, s2, s2, s2):
        acc = np.float32(acc + s)
    mean = np.float32(acc / np.float32(8))
    q = int(np.float32(mean * SR.qscale_of(0.375)))
    keep = torch.full((n,), MARK_K, dtype=torch.uint8, device="cuda")
    dist = torch.full((n,), float(MARK_F), dtype=torch.float32, device="cuda")
    idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    pts = torch.full((n, 3), float(MARK_F), dtype=torch.float32, device="cuda")
    before = dx.clone()
    torch.cuda.synchronize()
    nk, st = e.statistical_outlier_device(dx.data_ptr(), None, None, n, 8, 1.0, 0.375, (0, 0, 0), keep.data_ptr(), dist.data_ptr(),
                                          pts.data_ptr(), None, idx.data_ptr())
    m = (H - 2) * (W - 2)
    assert nk == m and st.tolist() == [n, 0, m, 2 * (H - 2) + 2 * (W - 2) + 4, m * q, m * q * q, q, 0]
    assert bool((keep == inner.to(torch.uint8)).all())
    assert bool((dist == torch.where(inner, torch.tensor(float(mean), device="cuda"), torch.tensor(-1.0, device="cuda"))).all())
    src = torch.nonzero(inner).reshape(-1).to(torch.int32)
    assert bool((idx[:m] == src).all()) and bool((idx[m:] == -1).all())
    assert bool((pts[:m] == dx[src.long()]).all()) and bool((pts[m:] == float(MARK_F)).all()) and bool((dx == before).all())


# ---- 8. guarded buffers -------------------------------------------------------------------------------------------------------------------
def test_the_cases_with_every_buffer_guarded():
    """(the same cases ran in the plain mode above)"""
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "statistical_guard_child.py")], capture_output=True, text=True, env=env,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"STATISTICAL_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) >= 14, tail
