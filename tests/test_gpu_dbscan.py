"""Density clustering on the device (needs an MI355X): sgm_cluster_dbscan, sgm_cluster_dbscan_device, Engine.cluster_dbscan_host /
_device, sgm.cluster_dbscan, sgm.largest_clusters.

Yardstick: tests/dbscan_ref.py -- the definition of include/sgm_hip_dbscan.h in numpy, over all pairs or over 27 cells -- bit for
bit: the labels, the core bytes, the sizes, the number of clusters and the six statistics exactly, through both entries.  Every
output is pre-filled with a marker, the rows of the sizes past the clusters must keep it, and every input is checked unmodified."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import covariance_ref as CR
import dbscan_ref as DR
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
NCASE = len(DR.SHAPE_CASES)
MARK_L, MARK_B, MARK_C, MARK_S, MARK_N = -77, 0xEE, 0xDEADBEEF, 0xABCDEF0123456789, -12345
ALL = ("labels", "core", "sizes", "stats")
GATHER, TIGHT, SOURCE = _lib.SGM_DBG_DBSCAN_GATHER_CORE, _lib.SGM_DBG_RADIUS_TIGHT_TABLE, _lib.SGM_DBG_RADIUS_SOURCE_ORDER


@pytest.fixture(scope="module")
def eng():
    return Engine(P16)


@functools.lru_cache(maxsize=None)
def layered():
    """the 24 x 130 layered cloud as lists (xyz, disp), shared and read-only"""
    return DR.layered_lists(24, 130, 724)


def host(e, xyz, disp, eps, k, o=(0, 0, 0), outs=ALL):
    """the host entry called on marked outputs: a dict of whole arrays (None where not asked for)"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    before = [xyz.copy(), None if disp is None else np.array(disp)]
    m = max(n, 1)
    g = dict(labels=np.full(m, MARK_L, np.int32) if "labels" in outs else None,
             core=np.full(m, MARK_B, np.uint8) if "core" in outs else None,
             sizes=np.full(m, MARK_C, np.uint32) if "sizes" in outs else None,
             stats=np.full(6, MARK_S, np.uint64) if "stats" in outs else None)
    org = np.asarray(o, np.float32)
    nc = C.c_int64(MARK_N)
    at = lambda a: None if a is None else a.ctypes.data
    rc = _lib.load().sgm_cluster_dbscan(e._h, xyz.ctypes.data, at(disp), n, float(eps), int(k), org.ctypes.data, at(g["labels"]),
                                        at(g["core"]), at(g["sizes"]), at(g["stats"]), C.byref(nc))
    assert rc == 0, _lib.last_error()
    assert np.array_equal(xyz, before[0], equal_nan=True) and (disp is None or np.array_equal(disp, before[1], equal_nan=True))
    return dict(g, n=n, n_clusters=int(nc.value))


def device(e, xyz, disp, eps, k, o=(0, 0, 0), outs=ALL):
    """the same through the device entry, every array a tensor of its own"""
    import torch
    dev = torch.device("cuda", e.device)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    dx, dd = up(xyz), up(disp)
    m = max(n, 1)
    t = dict(labels=torch.full((m,), MARK_L, dtype=torch.int32, device=dev) if "labels" in outs else None,
             core=torch.full((m,), MARK_B, dtype=torch.uint8, device=dev) if "core" in outs else None,
             sizes=torch.from_numpy(np.full(m, MARK_C, np.uint32).view(np.int32)).to(dev) if "sizes" in outs else None)
    p = lambda x: None if x is None else x.data_ptr()
    org = np.asarray(o, np.float32)
    st = np.full(6, MARK_S, np.uint64) if "stats" in outs else None
    nc = C.c_int64(MARK_N)
    torch.cuda.synchronize()
    rc = _lib.load().sgm_cluster_dbscan_device(e._h, p(dx), p(dd), n, float(eps), int(k), org.ctypes.data, p(t["labels"]), p(t["core"]),
                                               p(t["sizes"]), None if st is None else st.ctypes.data, C.byref(nc))
    assert rc == 0, _lib.last_error()
    e.synchronize()
    assert np.array_equal(dx.cpu().numpy(), xyz, equal_nan=True) and (disp is None or np.array_equal(dd.cpu().numpy(), disp, equal_nan=True))
    g = {k_: None if x is None else x.cpu().numpy() for k_, x in t.items()}
    g["sizes"] = None if g["sizes"] is None else g["sizes"].view(np.uint32)
    return dict(g, stats=st, n=n, n_clusters=int(nc.value))


def same(got, want, what=""):
    """bit for bit against a reference result"""
    n, nc = got["n"], want["n_clusters"]
    assert got["n_clusters"] == nc, (what, got["n_clusters"], nc)
    if got["stats"] is not None:
        assert got["stats"].dtype == np.uint64 and got["stats"].tolist() == want["stats"].tolist(), (what, got["stats"], want["stats"])
    if got["labels"] is not None:
        bad = np.nonzero(got["labels"][:n] != want["labels"])[0]
        assert got["labels"].dtype == np.int32 and bad.size == 0, (what, "labels", bad.size, bad[:5], got["labels"][bad[:5]], want["labels"][bad[:5]])
    if got["core"] is not None:
        assert got["core"].dtype == np.uint8 and np.array_equal(got["core"][:n], want["core"]), (what, "core")
    if got["sizes"] is not None:
        assert got["sizes"].dtype == np.uint32 and np.array_equal(got["sizes"][:nc], want["sizes"]), (what, "sizes", got["sizes"][:nc], want["sizes"])
        assert (got["sizes"][nc:] == MARK_C).all(), (what, "the rows past the clusters")


def both(e, xyz, disp, eps, k, o=(0, 0, 0), want=None, what=""):
    if want is None:
        want = DR.cells(np.asarray(xyz, np.float32).reshape(-1, 3), disp, eps, k, o)
    same(host(e, xyz, disp, eps, k, o), want, (what, "host"))
    same(device(e, xyz, disp, eps, k, o), want, (what, "device"))
    return want


def bytes_of(g):
    return [None if g[k] is None else g[k].tobytes() for k in ALL] + [g["n_clusters"]]


def stats(w):
    return dict(zip(DR.STATS, (int(x) for x in w["stats"])))


# ---- 1. shapes, through both entries, with and without disp, each optional output ------------------------------------------------------
@pytest.mark.parametrize("i", range(NCASE))
def test_shapes_through_both_entries(eng, i):
    eps, k, o = DR.SHAPE_CASES[i][3:]
    xyz, disp = DR.case_input(i)
    for with_disp in ((True, False) if disp is not None else (False,)):
        want = DR.case_want(i, with_disp)
        for fn in (host, device):
            same(fn(eng, xyz, disp if with_disp else None, eps, k, o), want, (i, fn.__name__, with_disp))
    want = DR.case_want(i)
    for out, fn in zip(ALL, (host, device, host, device)):           # each output alone, and none at all
        same(fn(eng, xyz, disp, eps, k, o, outs=(out,)), want, (i, "only", out))
    for out, fn in zip(ALL, (device, host, device, host)):
        same(fn(eng, xyz, disp, eps, k, o, outs=(out,)), want, (i, "only", out))
    same(host(eng, xyz, disp, eps, k, o, outs=()), want, (i, "no outputs"))
    same(device(eng, xyz, disp, eps, k, o, outs=()), want, (i, "no outputs"))


def test_the_layered_rows_are_no_trivial_clouds():
    """(asserted on the reference alone in tests/test_dbscan_reference.py; here so that this file cannot pass without it)"""
    good = sum(s["clusters"] >= 3 and min(s["core"], s["border"], s["noise"]) >= 0.05 * s["in_range"]
               for s in (stats(DR.case_want(i)) for i in DR.LAYERED_ROWS))
    assert good >= 3


def test_an_xyz_image_with_its_disparities(eng):
    """the 48 x 320 image: the points without a disparity are in no cell and are noise"""
    xyz, disp = DR.case_input(8)
    want = DR.case_want(8)
    s = stats(want)
    assert s["in_range"] < xyz.shape[0]
    g = device(eng, xyz.reshape(48, 320, 3), disp, *DR.SHAPE_CASES[8][3:])
    same(g, want, "image")
    out = ~want["in_range"]
    assert (g["labels"][out] == -1).all() and (g["core"][out] == 0).all()


# ---- 2. geometry in closed form -----------------------------------------------------------------------------------------------------
def test_pairs_borders_and_links_straddling_every_face_edge_and_corner(eng):
    """per direction a pair on either side of that face, edge or corner of a cell, a third point beside the first and a fourth 0.2
    beyond the second, within eps of it alone.  k = 1: every four are a cluster of core points, a link of it crossing the face.
    k = 2: the first three are core and the fourth is a border point whose only core point lies across the face from the rest.
    k = 3: the second point alone is core, with three border points on both sides of the face."""
    for origin in ((0.0, 0.0, 0.0), (0.3, -1.7, 2.2)):
        pairs, dirs = RR.face_pairs(0.25, origin)
        third = pairs[0::2] + np.float32(0.02) * np.roll(dirs, 1, axis=1).astype(np.float32) + np.float32([0.005, 0.01, -0.0075])
        unit = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
        fourth = pairs[1::2] + (0.2 * unit).astype(np.float32)
        xyz = np.concatenate([pairs, third.astype(np.float32), fourth.astype(np.float32)])
        assert len(dirs) == 26
        w = both(eng, xyz, None, 0.25, 1, origin, what="faces k=1")
        assert w["n_clusters"] == 26 and (w["sizes"] == 4).all() and w["core"].all()
        w = both(eng, xyz, None, 0.25, 2, origin, what="faces k=2")
        assert w["n_clusters"] == 26 and (w["sizes"] == 4).all() and stats(w)["border"] == 26 and not w["core"][78:].any()
        assert np.array_equal(w["labels"][78:], w["labels"][1:52:2])              # each border point with the point across the face
        w = both(eng, xyz, None, 0.25, 3, origin, what="faces k=3")
        assert stats(w)["core"] == 26 and w["core"][1:52:2].all() and w["n_clusters"] == 26 and (w["sizes"] == 4).all()


def test_the_long_diagonal_chain_and_two_chains_an_ulp_apart(eng):
    """3000 points spaced 0.9 eps along (1, 1, 1): a tree 3000 links deep across hundreds of cells and a dozen workgroups; and two
    such chains whose closest points are one ulp beyond eps, then one ulp nearer"""
    a, b = DR.two_chains(3000, 0.1)
    w = both(eng, a, None, 0.1, 1, what="chain k=1")
    assert w["sizes"].tolist() == [3000] and (w["labels"] == 0).all()
    w = both(eng, a, None, 0.1, 2, what="chain k=2")
    assert w["sizes"].tolist() == [3000] and stats(w)["border"] == 2
    two = np.concatenate([a, b])
    w = both(eng, two, None, 0.1, 1, what="two chains")
    assert w["sizes"].tolist() == [3000, 3000] and w["labels"].tolist() == [0] * 3000 + [1] * 3000
    nearer = np.array(two)
    nearer[3000, 0] = np.nextafter(nearer[3000, 0], np.float32(1))
    w = both(eng, nearer, None, 0.1, 1, what="two chains joined")
    assert w["sizes"].tolist() == [6000]
    perm = np.random.default_rng(5).permutation(6000)                # the indices shuffled along the chains: the links point everywhere
    w = both(eng, two[perm], None, 0.1, 1, what="two chains shuffled")
    assert sorted(w["sizes"].tolist()) == [3000, 3000] and len(set(w["labels"][np.argsort(perm)][:3000].tolist())) == 1
    w = both(eng, two[::-1].copy(), None, 0.1, 2, what="two chains reversed")
    assert w["sizes"].tolist() == [3000, 3000] and stats(w)["border"] == 4


def test_4096_identical_points(eng):
    xyz = np.tile(np.array([[0.3, -0.2, 1.7]], np.float32), (4096, 1))
    want = dict(labels=np.zeros(4096, np.int32), core=np.ones(4096, np.uint8), sizes=np.array([4096], np.uint32), n_clusters=1,
                stats=np.array([4096, 0, 4096, 0, 0, 1], np.uint64))
    both(eng, xyz, None, 0.05, 1, want=want, what="k = 1")
    both(eng, xyz, None, 0.05, 4095, want=want, what="k = 4095")
    noise = dict(labels=np.full(4096, -1, np.int32), core=np.zeros(4096, np.uint8), sizes=np.zeros(0, np.uint32), n_clusters=0,
                 stats=np.array([4096, 0, 0, 0, 4096, 0], np.uint64))
    both(eng, xyz, None, 0.05, 4096, want=noise, what="k = 4096")


def test_a_4097_point_cell_between_two_runs(eng):
    """4097 points in one cell between runs of 301 and 303 points in the cells beside it: the run loop goes far past RAD_RUN_LOADS
    with ragged ends, and one workgroup's lanes unite into one tree"""
    rng = np.random.default_rng(8)
    v = float(np.float32(0.4) * np.float32(1.03125))
    mid = (rng.random((4097, 3)) * 0.9 + 0.05) * v + np.array([2 * v, 0, 0])
    left = (rng.random((301, 3)) * 0.9 + 0.05) * v + np.array([1 * v, 0, 0])
    right = (rng.random((303, 3)) * 0.9 + 0.05) * v + np.array([3 * v, 0, 0])
    xyz = np.concatenate([left, mid, right]).astype(np.float32)
    want = both(eng, xyz, None, 0.4, 3, what="one cell")
    assert want["sizes"].tolist() == [4701]
    want = both(eng, xyz, None, 0.4, 3000, what="one cell, k = 3000")
    assert 0 < stats(want)["core"] < 4701 and stats(want)["border"] > 0


def test_the_equidistant_border_tie(eng):
    def clump(tip, sign):
        x = tip + sign * 0.125
        return [[tip, 0, 0], [x, 0.0625, 0], [x, -0.0625, 0], [x, 0, 0.0625]]
    left, right, mid = clump(-0.1875, -1), clump(0.1875, 1), [[0, 0, 0]]
    for pts, labels in ((left + right + mid, [0] * 4 + [1] * 4 + [0]), (right + left + mid, [0] * 4 + [1] * 4 + [0]),
                        (mid + right + left, [0] * 5 + [1] * 4), (left[::-1] + mid + right[::-1], [0] * 5 + [1] * 4),
                        (right[::-1] + mid + left[::-1], [0] * 5 + [1] * 4)):
        w = both(eng, np.float32(pts), None, 0.25, 3, what="tie")
        assert w["labels"].tolist() == labels and stats(w)["border"] == 1
    # 300 such border points at once, each between its own two clumps, the lower index alternately on the left and on the right
    rows = []
    for t in range(300):
        shift = np.float32([0, 4.0 * t, 0])
        l, r = np.float32(clump(-0.1875, -1)) + shift, np.float32(clump(0.1875, 1)) + shift
        rows += [l, r, shift[None, :]] if t % 2 == 0 else [r, l, shift[None, :]]
    w = both(eng, np.concatenate(rows), None, 0.25, 3, what="300 ties")
    assert w["n_clusters"] == 600 and sorted(set(w["sizes"].tolist())) == [4, 5] and w["sizes"][0::2].tolist() == [5] * 300


def test_all_invalid_and_all_out_of_range(eng):
    xyz, disp = layered()
    n = xyz.shape[0]
    w = both(eng, xyz, np.zeros(n, np.float32), 0.05, 3, what="disp 0")
    assert w["stats"].tolist() == [0] * 6 and (w["labels"] == -1).all() and (w["core"] == 0).all()
    bad = np.array(xyz)
    bad[np.arange(n), np.arange(n) % 3] = np.nan
    assert both(eng, bad, None, 0.05, 3, what="nan")["stats"].tolist() == [0] * 6
    w = both(eng, np.full((n, 3), 3e38, np.float32), None, 1.0, 3, what="all out of range")
    assert w["stats"].tolist() == [0, n, 0, 0, 0, 0] and (w["labels"] == -1).all()
    far = np.array(xyz)
    far[5::7, 0] = 3.0e5
    w = both(eng, far, disp, 0.05, 8, what="some out of range")
    assert stats(w)["out_of_range"] > 300 and stats(w)["clusters"] >= 3 and (w["labels"][~w["in_range"]] == -1).all()


def test_negative_coordinates_and_an_origin(eng):
    xyz, disp = layered()
    neg = -np.abs(np.array(xyz)) - np.float32(0.37)
    w = both(eng, neg, disp, 0.05, 8, (0.013, -2.5, 100.0), what="negative")
    assert stats(w)["clusters"] >= 3 and stats(w)["border"] > 20 and stats(w)["noise"] > 10
    a = both(eng, xyz, disp, 0.05, 8, (0.013, -2.5, 100.0), what="origin")
    b = both(eng, xyz, disp, 0.05, 8, what="no origin")
    assert np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["sizes"], b["sizes"])      # (in range either way: the origin shows nowhere)


@pytest.mark.parametrize("e", [40, -40])
def test_a_cloud_scaled_by_a_power_of_two(eng, e):
    s = np.float32(2.0) ** e
    xyz, disp = layered()
    want = DR.want_of("layered", xyz, disp, 0.05, 8)
    both(eng, xyz * s, disp, float(np.float32(0.05) * s), 8, want=want, what=e)


# ---- 3. determinism, engine state ----------------------------------------------------------------------------------------------------
def test_the_debug_bits_give_the_same_bits():
    """the core bit gathered by source index, alone and with the table at the tight size and the radius filter's source order bit:
    the bytes of the default on the shape cases and on the chains"""
    e = Engine(P16)
    runs = [(DR.case_input(i), DR.SHAPE_CASES[i][3:], DR.case_want(i)) for i in range(NCASE)]
    a, b = DR.two_chains(3000, 0.1)
    two = np.concatenate([a, b])
    runs.append(((two, None), (0.1, 2, (0, 0, 0)), DR.want_of("two chains", two, None, 0.1, 2)))
    plain = [bytes_of(host(e, *inp, *par)) for inp, par, _ in runs]
    try:
        for bits in (GATHER, TIGHT, SOURCE, GATHER | TIGHT, GATHER | SOURCE, GATHER | TIGHT | SOURCE):
            e.set_option(_lib.SGM_OPT_DEBUG, bits)
            for (inp, par, want), first in zip(runs, plain):
                g = host(e, *inp, *par)
                same(g, want, (bits, par))
                assert bytes_of(g) == first
                same(device(e, *inp, *par), want, (bits, par, "device"))
    finally:
        e.set_option(_lib.SGM_OPT_DEBUG, 0)


def test_five_calls_give_the_same_bytes(eng):
    xyz, disp = DR.case_input(9)
    par = DR.SHAPE_CASES[9][3:]
    runs = [bytes_of(device(eng, xyz, disp, *par)) for _ in range(5)]
    assert all(r == runs[0] for r in runs[1:])
    same(device(eng, xyz, disp, *par), DR.case_want(9))
    runs = [bytes_of(host(eng, xyz, disp, *par)) for _ in range(5)]
    assert all(r == runs[0] for r in runs[1:])


def _others(e):
    """the two outlier removals and the covariance normals on engine e, each held against its reference"""
    def radius(i):
        xyz, disp, col = RR.case_input(i)
        r, nb, mc, o = RR.SHAPE_CASES[i][3:]
        w = RR.case_want(i)
        p, c, keep, cnt, idx, noor = e.radius_outlier_host(xyz, disp, col, r, nb, mc, o, return_counts=True, return_index=True)
        assert np.array_equal(keep, w["keep"]) and np.array_equal(cnt, w["counts"]) and np.array_equal(idx, w["index"])
        assert np.array_equal(p.view(np.uint32), w["points"].view(np.uint32))

    def statistical(i):
        xyz, disp, col = SR.case_input(i)
        k, ratio, r, o = SR.SHAPE_CASES[i][3:]
        w = SR.case_want(i)
        p, c, keep, mean, idx, st = e.statistical_outlier_host(xyz, disp, col, k, ratio, r, o, return_distances=True)
        assert np.array_equal(keep, w["keep"]) and np.array_equal(mean.view(np.uint32), w["mean"].view(np.uint32)) and st.tolist() == w["stats"].tolist()

    def covariance(i):
        xyz, disp = CR.case_input(i)
        w = CR.case_want(i)
        nrm, curv, cnt, st = e.covariance_normals_host(xyz, disp, *CR.SHAPE_CASES[i][3:], return_curvature=True, return_counts=True)
        assert np.array_equal(nrm.view(np.uint32), w["normals"].view(np.uint32)) and np.array_equal(cnt, w["counts"]) and st.tolist() == w["stats"].tolist()
    return radius, statistical, covariance


def test_a_long_lived_engine_from_poisoned_buffers():
    """clustering, radius, statistical and covariance calls interleaved at changing n on one engine whose buffers start as 0xA5 / 0x7F"""
    e = Engine(P16)
    radius, statistical, covariance = _others(e)

    def db(i, fn):
        xyz, disp = DR.case_input(i)
        same(fn(e, xyz, disp, *DR.SHAPE_CASES[i][3:]), DR.case_want(i), (i, fn.__name__))
    try:
        for byte in (0xA5, 0x7F):
            e.set_option(_lib.SGM_OPT_POISON, byte)      # fills every buffer the engine owns and arms the same for new ones
            db(8, host)
            radius(7)                                    # 48 x 320: the same table, the records without a core bit
            db(10, device)
            e.set_option(_lib.SGM_OPT_POISON, byte)
            statistical(6)
            db(4, device)                                # 65 points in the larger table
            covariance(7)
            db(9, host)
            e.trim()                                     # gives the table, the links and the staged outputs back
            db(6, host)
            radius(5)
            db(2, device)
        e.set_option(_lib.SGM_OPT_DEBUG, GATHER)
        e.set_option(_lib.SGM_OPT_POISON, 0xA5)
        db(9, host)
        db(5, device)
    finally:
        e.set_option(_lib.SGM_OPT_POISON, -1)
        e.set_option(_lib.SGM_OPT_DEBUG, 0)


def test_the_profile_record_names_the_stages():
    e = Engine(P16)
    xyz, disp = DR.case_input(9)
    par = DR.SHAPE_CASES[9][3:]
    want = {"dbscan_count": 1, "dbscan_clear": 1, "dbscan_insert": 1, "dbscan_starts": 1, "dbscan_sort": 1, "dbscan_core": 2,
            "dbscan_link": 1, "dbscan_number": 3, "dbscan_label": 1, "_wall": 0}
    try:
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        for bits in (0, GATHER):
            e.set_option(_lib.SGM_OPT_DEBUG, bits)
            same(device(e, xyz, disp, *par), DR.case_want(9))
            st = {n: launches for n, ms, launches in e.stage_times()}
            assert st == want and tuple(n for n, ms, k in e.stage_times() if n != "_wall") == _lib.DBSCAN_STAGES, st
            assert all(ms >= 0 for n, ms, k in e.stage_times())
        same(host(e, xyz, np.zeros_like(disp), *par), DR.cells(xyz, np.zeros_like(disp), *par))       # nothing arrives: the count alone
        assert {n: k for n, ms, k in e.stage_times()} == {"dbscan_count": 1, "_wall": 0}
    finally:
        e.set_option(_lib.SGM_OPT_PROFILE, 0)
        e.set_option(_lib.SGM_OPT_DEBUG, 0)


def test_refusals_leave_the_outputs_untouched_and_the_engine_usable(eng):
    L = _lib.load()
    xyz = np.array(layered()[0][:100])
    n = 100
    lab, core, sizes = np.full(n, MARK_L, np.int32), np.full(n, MARK_B, np.uint8), np.full(n, MARK_C, np.uint32)
    st = np.full(6, MARK_S, np.uint64)
    nc = C.c_int64(MARK_N)
    org, nan3 = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(0, float("nan"), 0)
    inf3 = (C.c_float * 3)(float("inf"), 0, 0)
    X = xyz.ctypes.data
    out = (lab.ctypes.data, core.ctypes.data, sizes.ctypes.data, st.ctypes.data)
    h = eng._h
    ref = C.byref(nc)
    bad = [(None, X, None, n, 0.05, 3, org) + out + (ref,), (h, None, None, n, 0.05, 3, org) + out + (ref,),
           (h, X, None, n, 0.05, 3, org) + out + (None,), (h, X, None, -1, 0.05, 3, org) + out + (ref,)]
    bad += [(h, X, None, n, 0.05, k, org) + out + (ref,) for k in (0, -3, 1 << 24, 1 << 30)]
    bad += [(h, X, None, n, r, 3, org) + out + (ref,) for r in (0.0, -1.0, float("nan"), float("inf"), 1e-45, 1e-20, 1e20)]
    bad += [(h, X, None, n, 0.05, 3, o) + out + (ref,) for o in (nan3, inf3, None)]
    for fn in (L.sgm_cluster_dbscan, L.sgm_cluster_dbscan_device):
        for args in bad:
            assert fn(*args) == -1, args                                   # SGM_ERR_INVALID_ARG
            assert b"sgm_cluster_dbscan" in L.sgm_last_error()
        assert fn(h, X, None, 1 << 24, 0.05, 3, org, *out, ref) == -4      # SGM_ERR_UNSUPPORTED: before anything is read
        assert b"2^24" in L.sgm_last_error()
    assert (lab == MARK_L).all() and (core == MARK_B).all() and (sizes == MARK_C).all() and (st == MARK_S).all() and nc.value == MARK_N
    # n = 0 succeeds with no cluster, the statistics zero and nothing else written
    for fn in (L.sgm_cluster_dbscan, L.sgm_cluster_dbscan_device):
        st[:] = MARK_S
        nc.value = MARK_N
        assert fn(h, X, None, 0, 0.05, 3, org, *out, ref) == 0 and st.tolist() == [0] * 6 and nc.value == 0
        assert fn(h, X, None, 0, 0.05, 3, org, None, None, None, None, ref) == 0
    assert (lab == MARK_L).all() and (core == MARK_B).all() and (sizes == MARK_C).all()
    a, b = layered()
    both(eng, a, b, 0.05, 8, want=DR.want_of("layered", a, b, 0.05, 8), what="after the refusals")


def test_the_other_cloud_calls_are_unchanged_with_clustering_calls_between_them():
    e = Engine(P16)
    xyz, disp, col = VR.layered_cloud(97, 331, 9)
    lst = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)

    def cluster():
        g = host(e, lst[0], lst[1], 0.02, 6)
        assert g["n_clusters"] >= 3 and 0 < g["stats"][3] and 0 < g["stats"][4]
        return bytes_of(g)
    first = cluster()
    w = RR.cells(*lst, 0.02, 8, 12)
    p, c, keep, cnt, idx, noor = e.radius_outlier_host(*lst, 0.02, 8, 12, return_counts=True, return_index=True)
    assert np.array_equal(keep, w["keep"]) and np.array_equal(cnt, w["counts"]) and np.array_equal(idx, w["index"]) and noor == w["n_out_of_range"]
    assert np.array_equal(p.view(np.uint32), w["points"].view(np.uint32)) and np.array_equal(c, w["colors"])
    assert cluster() == first
    w = SR.cells(*lst, 8, 1.0, 0.03)
    p, c, keep, mean, idx, st = e.statistical_outlier_host(*lst, 8, 1.0, 0.03, return_distances=True, return_index=True)
    assert np.array_equal(keep, w["keep"]) and np.array_equal(mean.view(np.uint32), w["mean"].view(np.uint32)) and st.tolist() == w["stats"].tolist()
    assert cluster() == first
    w = CR.cells(lst[0], lst[1], 0.03, 5)
    nrm, curv, cnt, st = e.covariance_normals_host(lst[0], lst[1], 0.03, 5, return_curvature=True, return_counts=True)
    assert np.array_equal(nrm.view(np.uint32), w["normals"].view(np.uint32)) and np.array_equal(cnt, w["counts"]) and st.tolist() == w["stats"].tolist()
    assert cluster() == first
    w = VR.voxel_downsample(*lst, 0.05, (0, 0, 0), 2)
    p, c, k, noor = e.voxel_downsample_host(*lst, 0.05, (0, 0, 0), 2, return_counts=True)
    assert np.array_equal(p.view(np.uint32), w["points"].view(np.uint32)) and np.array_equal(c, w["colors"]) and np.array_equal(k, w["counts"])
    assert cluster() == first
    same(host(e, lst[0], lst[1], 0.02, 6), DR.cells(lst[0], lst[1], 0.02, 6), "97 x 331")


# ---- 4. the Python surface -------------------------------------------------------------------------------------------------------------
def test_cluster_dbscan_on_numpy_input_and_on_tensors():
    import torch
    xyz, disp = DR.case_input(8)
    col = np.random.default_rng(2).integers(0, 256, size=(48, 320, 3), dtype=np.uint8)
    img = np.array(xyz).reshape(48, 320, 3)
    dmap = np.array(disp).reshape(48, 320)
    eps, k, o = DR.SHAPE_CASES[8][3:]
    want = DR.case_want(8)
    lab = sgm.cluster_dbscan(img, dmap, eps, k)
    assert lab.shape == (48, 320) and lab.dtype == np.int32 and np.array_equal(lab.reshape(-1), want["labels"])
    lab, core, sizes, st = sgm.cluster_dbscan(img, dmap, eps, k, return_core=True, return_sizes=True, return_stats=True)
    assert core.shape == (48, 320) and core.dtype == np.uint8 and sizes.dtype == np.uint32 and st == stats(want)
    assert np.array_equal(core.reshape(-1), want["core"]) and np.array_equal(sizes, want["sizes"])
    # the mask of the two largest clusters as a confidence map of valid_points and triangulate_points
    mask = sgm.largest_clusters(lab, sizes, count=2, min_size=10)
    top = np.argsort(-want["sizes"].astype(np.int64), kind="stable")[:2]
    assert mask.shape == (48, 320) and np.array_equal(mask.reshape(-1) > 0, np.isin(want["labels"], top))
    pts, cols = sgm.valid_points(img, col, dmap, confidence=mask, min_confidence=1)
    sel = mask.reshape(-1) > 0
    assert pts.shape[0] == int(want["sizes"][top].sum()) and np.array_equal(pts.view(np.uint32), np.array(xyz)[sel].view(np.uint32))
    assert np.array_equal(cols, col.reshape(-1, 3)[sel])
    v, c, f = sgm.triangulate_points(img, col, dmap, 1.0, confidence=mask, min_confidence=1)
    v0, c0, f0 = sgm.triangulate_points(img, col, np.where(mask > 0, dmap, np.float32(0)), 1.0)
    assert np.array_equal(v.view(np.uint32), v0.view(np.uint32)) and np.array_equal(f, f0) and 0 < v.shape[0] <= pts.shape[0]
    # a list, another origin, a confidence map
    w2 = DR.cells(xyz, None, 0.02, 6, (0.5, 0.5, 0.5))
    l2, s2 = sgm.cluster_dbscan(np.array(xyz), None, 0.02, 6, origin=(0.5, 0.5, 0.5), return_sizes=True)
    assert l2.shape == (15360,) and np.array_equal(l2, w2["labels"]) and np.array_equal(s2, w2["sizes"])
    conf = np.random.default_rng(3).integers(0, 101, size=dmap.shape).astype(np.uint8)
    w3 = DR.cells(xyz, np.where(conf >= 40, dmap, np.float32(0)).reshape(-1), 0.02, 4)
    l3 = sgm.cluster_dbscan(img, dmap, 0.02, 4, confidence=conf, min_confidence=40)
    assert w3["n_clusters"] >= 3 and np.array_equal(l3.reshape(-1), w3["labels"])
    # HIP tensors stay on the device
    ti, td = torch.from_numpy(img).cuda(), torch.from_numpy(dmap).cuda()
    tl, tc, ts, tst = sgm.cluster_dbscan(ti, td, eps, k, return_core=True, return_sizes=True, return_stats=True)
    assert tl.is_cuda and tl.shape == (48, 320) and tl.dtype == torch.int32 and tc.dtype == torch.uint8 and tst == stats(want)
    assert np.array_equal(tl.cpu().numpy().reshape(-1), want["labels"]) and np.array_equal(tc.cpu().numpy().reshape(-1), want["core"])
    assert ts.shape == (want["n_clusters"],) and np.array_equal(ts.cpu().numpy(), want["sizes"].view(np.int32))
    tm = sgm.largest_clusters(tl, ts, count=2, min_size=10)
    assert tm.is_cuda and tm.dtype == torch.uint8 and np.array_equal(tm.cpu().numpy(), mask)
    tl2 = sgm.cluster_dbscan(torch.from_numpy(np.array(xyz)).cuda(), None, 0.02, 6, origin=(0.5, 0.5, 0.5))
    assert tl2.is_cuda and np.array_equal(tl2.cpu().numpy(), w2["labels"])
    t3 = sgm.cluster_dbscan(ti, td, 0.02, 4, confidence=torch.from_numpy(conf).cuda(), min_confidence=40)
    assert np.array_equal(t3.cpu().numpy().reshape(-1), w3["labels"])
    with pytest.raises(sgm.error, match="float32 and on the GPU"):
        sgm.cluster_dbscan(torch.from_numpy(img), td, 0.02, 4)
    with pytest.raises(sgm.error, match="same GPU"):
        sgm.cluster_dbscan(ti, dmap, 0.02, 4)


def test_the_centroids_of_a_270_x_480_frame():
    """270 x 480 through sgm_pipeline_device, voxel_down_sample, cluster_dbscan at twice the voxel size, largest_clusters: the chain
    the call exists for"""
    import torch
    H, W, D = 270, 480, 64
    a, b = synth.make_pair(H, W, D, seed=5)[:2]
    e = Engine(U.params(D, 5, 0, 1))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dd = torch.empty((H, W), dtype=torch.int16, device="cuda")
    df = torch.empty((H, W), dtype=torch.float32, device="cuda")
    dx = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, synth.default_Q(W), dd.data_ptr(), df.data_ptr(), dx.data_ptr())
    e.synchronize()
    xyz, disp = dx.cpu().numpy(), df.cpu().numpy()
    rgb = np.repeat(a[:, :, None], 3, axis=2) ^ np.array([0, 85, 170], np.uint8)
    ok = np.isfinite(xyz).all(axis=2) & (disp > 0)
    with np.errstate(all="ignore"):
        step = float(np.median(np.abs(xyz[:, 1:, 0] - xyz[:, :-1, 0])[ok[:, 1:] & ok[:, :-1]]))
    voxel = float(np.float32(6 * step))
    cen, col = sgm.voxel_down_sample(xyz, rgb, disp, voxel)
    assert 1000 < cen.shape[0] < 20000, cen.shape
    eps = float(np.float32(2) * np.float32(voxel))
    want = DR.cells(cen, None, eps, 4)
    s = stats(want)
    assert s["clusters"] >= 1 and s["core"] > 0.25 * s["in_range"], s
    lab, core, sizes, st = sgm.cluster_dbscan(cen, None, eps, 4, return_core=True, return_sizes=True, return_stats=True)
    assert st == s and np.array_equal(lab, want["labels"]) and np.array_equal(core, want["core"]) and np.array_equal(sizes, want["sizes"])
    mask = sgm.largest_clusters(lab, sizes)
    assert int(mask.sum()) == int(sizes.max()) and (lab[mask > 0] == int(np.argmax(sizes))).all()


# ---- 5. full size ----------------------------------------------------------------------------------------------------------------------
def test_a_full_size_planar_lattice_in_stripes():
    """2160 x 4096 points at spacing 0.25 in the plane Z = 2 with every 64th row (63, 127, ...) invalid through its disparity,
    eps just above the spacing, min_points = 2: every point left has at least two neighbours in its row, rows a step apart are
    linked and rows two steps apart are not, so the clusters are the stripes of 63 rows (the last of 48: 2160 = 33 * 64 + 48 and row
    2175 would be the next to go), in the order of the rows.  8.7 M points in the largest table the call can need (2^25 slots); 258 048 points per tree."""
    import torch
    H, W = 2160, 4096
    n = H * W
    e = Engine(P16)
    y, x = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    dx = torch.stack([x * 0.25 - 300.0, y * 0.25 - 100.0, torch.full_like(x, 2.0)], dim=2).reshape(n, 3).contiguous()
    row = torch.arange(H, device="cuda").repeat_interleave(W)
    del x, y
    gone = (row % 64) == 63
    disp = torch.where(gone, torch.tensor(0.0, device="cuda"), torch.tensor(1.0, device="cuda")).contiguous()
    lab = torch.full((n,), MARK_L, dtype=torch.int32, device="cuda")
    core = torch.full((n,), MARK_B, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    before = dx.clone()
    torch.cuda.synchronize()
    nc, st = e.cluster_dbscan_device(dx.data_ptr(), disp.data_ptr(), n, 0.2578125, 2, (0, 0, 0), lab.data_ptr(), core.data_ptr(), sizes.data_ptr())
    rows_gone = H // 64
    assert nc == 34 and st.tolist() == [n - rows_gone * W, 0, n - rows_gone * W, 0, 0, 34], (nc, st)
    assert sizes[:34].tolist() == [63 * W] * 33 + [48 * W] and bool((sizes[34:] == -1).all())
    want = torch.where(gone, torch.tensor(-1, device="cuda"), (row // 64)).to(torch.int32)
    assert bool((lab == want).all()) and bool((core == (~gone).to(torch.uint8)).all())
    assert bool((dx == before).all())
    mask = sgm.largest_clusters(lab, sizes[:34], count=33)
    assert int(mask.sum()) == 33 * 63 * W and not bool(mask[row >= 33 * 64].any())


# ---- 6. guarded buffers -------------------------------------------------------------------------------------------------------------------
def test_the_cases_with_every_buffer_guarded():
    """(the same cases ran in the plain mode above)"""
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dbscan_guard_child.py")], capture_output=True, text=True, env=env,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"DBSCAN_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) >= 6, tail
