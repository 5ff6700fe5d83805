"""Plane segmentation on the device (needs an MI355X): sgm_segment_plane, sgm_segment_plane_device, sgm_plane_inliers,
sgm_plane_inliers_device, Engine.segment_plane_host / _device, Engine.plane_inliers_host / _device, sgm.segment_plane,
sgm.plane_inliers.

Yardstick: tests/plane_ref.py -- the definition of include/sgm_hip_plane.h in numpy, with the fused multiply-add emulated exactly --
bit for bit: the model, the inlier bytes, the distances, the compacted points, colours and indices as uint32 / uint8, both counts
and the eight statistics (k* and its count among them), through both entries and under both forms of the counting kernel
(SGM_DBG_PLANE_OTHER_COUNT).  Every output is pre-filled with a marker, the rows past the selected points must keep it, and every
input is checked unmodified."""
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
import plane_ref as PR
import radius_ref as RR
import voxel_ref as VR
import stereo_reconstruction_cv_amd as sgm
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = dict(numDisparities=16)
NCASE = len(PR.SHAPE_CASES)
MARK_B, MARK_F, MARK_I, MARK_S, MARK_N = 0xEE, 0xC2F6E979, 0xDEADBEEF, 0xABCDEF0123456789, -12345
ALL = ("inlier", "distance", "points", "colors", "index", "model", "stats")
OTHER = _lib.SGM_DBG_PLANE_OTHER_COUNT
F32 = np.float32


@pytest.fixture(scope="module")
def eng():
    return Engine(P16)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _marked(n, outs, colors):
    m = max(n, 1)
    fl = lambda shape: np.full(shape, MARK_F, np.uint32).view(np.float32)
    return dict(inlier=np.full(m, MARK_B, np.uint8) if "inlier" in outs else None,
                distance=fl(m) if "distance" in outs else None,
                points=fl((m, 3)) if "points" in outs else None,
                colors=np.full((m, 3), MARK_B, np.uint8) if "colors" in outs and colors is not None else None,
                index=np.full(m, MARK_I, np.uint32) if "index" in outs else None,
                model=fl(4) if "model" in outs else None,
                stats=np.full(8, MARK_S, np.uint64) if "stats" in outs else None)


def host(e, xyz, disp, colors, t, K, seed, refine=1, select=0, outs=ALL, model=None):
    """the host entry called on marked outputs (model given: sgm_plane_inliers): a dict of whole arrays (None where not asked for)"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    before = [xyz.copy(), None if disp is None else np.array(disp), None if colors is None else np.array(colors)]
    g = _marked(n, outs, colors)
    ni, ns = C.c_int64(MARK_N), C.c_int64(MARK_N)
    at = lambda a: None if a is None else a.ctypes.data
    L = _lib.load()
    if model is None:
        rc = L.sgm_segment_plane(e._h, xyz.ctypes.data, at(disp), at(colors), n, float(t), int(K), int(seed), int(refine), int(select),
                                 at(g["inlier"]), at(g["distance"]), at(g["points"]), at(g["colors"]), at(g["index"]), at(g["model"]),
                                 at(g["stats"]), C.byref(ni), C.byref(ns))
    else:
        mod = np.ascontiguousarray(model, np.float32)
        g["model"] = g["stats"] = None
        rc = L.sgm_plane_inliers(e._h, xyz.ctypes.data, at(disp), at(colors), n, mod.ctypes.data, float(t), int(select), at(g["inlier"]),
                                 at(g["distance"]), at(g["points"]), at(g["colors"]), at(g["index"]), C.byref(ni), C.byref(ns))
    assert rc == 0, _lib.last_error()
    assert np.array_equal(xyz, before[0], equal_nan=True) and (disp is None or np.array_equal(disp, before[1], equal_nan=True))
    assert colors is None or np.array_equal(colors, before[2])
    return dict(g, n=n, n_inliers=int(ni.value), n_selected=int(ns.value))


def device(e, xyz, disp, colors, t, K, seed, refine=1, select=0, outs=ALL, model=None):
    """the same through the device entry, every array a tensor of its own"""
    import torch
    dev = torch.device("cuda", e.device)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    dx, dd, dc = up(xyz), up(disp), up(colors)
    g = _marked(n, outs, colors)
    upi = lambda a: None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype in (np.uint32, np.float32) else a).to(dev)
    t_ = {k: upi(g[k]) for k in ("inlier", "distance", "points", "colors", "index")}
    p = lambda x: None if x is None else x.data_ptr()
    at = lambda a: None if a is None else a.ctypes.data
    ni, ns = C.c_int64(MARK_N), C.c_int64(MARK_N)
    L = _lib.load()
    torch.cuda.synchronize()
    if model is None:
        rc = L.sgm_segment_plane_device(e._h, p(dx), p(dd), p(dc), n, float(t), int(K), int(seed), int(refine), int(select), p(t_["inlier"]),
                                        p(t_["distance"]), p(t_["points"]), p(t_["colors"]), p(t_["index"]), at(g["model"]), at(g["stats"]),
                                        C.byref(ni), C.byref(ns))
    else:
        mod = np.ascontiguousarray(model, np.float32)
        g["model"] = g["stats"] = None
        rc = L.sgm_plane_inliers_device(e._h, p(dx), p(dd), p(dc), n, mod.ctypes.data, float(t), int(select), p(t_["inlier"]),
                                        p(t_["distance"]), p(t_["points"]), p(t_["colors"]), p(t_["index"]), C.byref(ni), C.byref(ns))
    assert rc == 0, _lib.last_error()
    e.synchronize()
    assert np.array_equal(dx.cpu().numpy(), xyz, equal_nan=True) and (disp is None or np.array_equal(dd.cpu().numpy(), disp, equal_nan=True))
    for k, x in t_.items():
        if x is not None:
            a = x.cpu().numpy()
            g[k] = a.view(np.float32) if k in ("distance", "points") else a.view(np.uint32) if k == "index" else a
    return dict(g, n=n, n_inliers=int(ni.value), n_selected=int(ns.value))


def same(got, want, what=""):
    """bit for bit against a reference result"""
    n, ns = got["n"], want["n_selected"]
    assert (got["n_inliers"], got["n_selected"]) == (want["n_inliers"], ns), (what, got["n_inliers"], got["n_selected"], want["n_inliers"], ns)
    if got["stats"] is not None:
        assert got["stats"].dtype == np.uint64 and got["stats"].tolist() == want["stats"].tolist(), (what, got["stats"], want["stats"])
    if got["model"] is not None:
        assert np.array_equal(u32(got["model"]), u32(want["model"])), (what, "model", got["model"], want["model"])
    if got["inlier"] is not None:
        assert got["inlier"].dtype == np.uint8 and np.array_equal(got["inlier"][:n], want["inlier"]), (what, "inlier")
    if got["distance"] is not None:
        bad = np.nonzero(u32(got["distance"][:n]) != u32(want["distance"]))[0]
        assert bad.size == 0, (what, "distance", bad.size, bad[:5], got["distance"][bad[:5]], want["distance"][bad[:5]])
    if got["points"] is not None:
        assert np.array_equal(u32(got["points"][:ns]), u32(want["points"])), (what, "points")
        assert (u32(got["points"][ns:]) == MARK_F).all(), (what, "the rows past the selected points")
    if got["colors"] is not None:
        assert np.array_equal(got["colors"][:ns], want["colors"]) and (got["colors"][ns:] == MARK_B).all(), (what, "colors")
    if got["index"] is not None:
        assert np.array_equal(got["index"][:ns], want["index"]) and (got["index"][ns:] == MARK_I).all(), (what, "index")


def bytes_of(g):
    return [None if g[k] is None else g[k].tobytes() for k in ALL] + [g["n_inliers"], g["n_selected"]]


def both_forms(e, fn):
    """fn() under the default counting kernel and under the other one"""
    try:
        for bits in (0, OTHER):
            e.set_option(_lib.SGM_OPT_DEBUG, bits)
            fn(bits)
    finally:
        e.set_option(_lib.SGM_OPT_DEBUG, 0)


def everything(e, xyz, disp, col, t, K, seed, refine=1, select=0, want=None, what=""):
    """host and device entry under both forms of the counting kernel against the reference"""
    if want is None:
        want = PR.segment(xyz, disp, col, t, K, seed, bool(refine), select)

    def run(bits):
        for fn in (host, device):
            same(fn(e, xyz, disp, col, t, K, seed, refine, select), want, (what, fn.__name__, bits))
    both_forms(e, run)
    return want


# ---- 1. shapes, through both entries and both forms, with and without disparities and colours, each optional output --------------------
@pytest.mark.parametrize("i", range(NCASE))
def test_shapes_through_both_entries(eng, i):
    t, K, seed, refine, select = PR.SHAPE_CASES[i][3:]
    xyz, disp, col = PR.case_input(i)
    everything(eng, xyz, disp, col, t, K, seed, refine, select, want=PR.case_want(i), what=i)
    if disp is not None:
        want = PR.case_want(i, False, False)
        for fn in (host, device):
            same(fn(eng, xyz, None, None, t, K, seed, refine, select), want, (i, fn.__name__, "a list"))
    want = PR.case_want(i)
    for out, fn in zip(ALL, (host, device) * 4):           # each output alone, and none at all
        same(fn(eng, xyz, disp, col, t, K, seed, refine, select, outs=(out,)), want, (i, "only", out))
    same(device(eng, xyz, disp, col, t, K, seed, refine, select, outs=()), want, (i, "no outputs"))


# ---- 2. the condition cases and the extremes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["layered", "tie", "duplicates", "refit_range"])
def test_the_condition_cases(eng, name):
    xyz, disp, col, t, K, seed = PR.condition_case(name)
    for select in (0, 1):
        everything(eng, xyz, disp, col, t, K, seed, 1, select, want=PR.want_of(name, xyz, disp, col, t, K, seed, True, select), what=name)
    everything(eng, xyz, disp, col, t, K, seed, 0, 0, want=PR.want_of(name, xyz, disp, col, t, K, seed, False, 0), what=(name, "no refit"))


def test_the_threshold_pair(eng):
    """points at exactly t and one ulp beyond, found by the fit itself and by sgm_plane_inliers"""
    t = F32(0.03)
    beyond = np.nextafter(t, F32(1))
    base = CR.plane_lattice(8, 8, 0.25, 0.0, 0.0, 0.0)
    extra = np.array([[0.1, 0.1, t], [0.3, 0.1, -t], [0.1, 0.3, beyond], [0.3, 0.3, -beyond]], np.float32)
    xyz = np.ascontiguousarray(np.concatenate([base, extra]))
    w = everything(eng, xyz, None, None, t, 32, 2, 0, 0, what="threshold")
    assert np.array_equal(u32(w["model"][:3]), u32(F32([0, 0, 1]))) and w["inlier"][-4:].tolist() == [1, 1, 0, 0]
    for fn in (host, device):
        for select in (0, 1):
            same(fn(eng, xyz, None, None, t, 0, 0, 0, select, model=[0, 0, 1, 0]), PR.classify(xyz, None, None, F32([0, 0, 1, 0]), t, select),
                 ("inliers", fn.__name__, select))


def test_extremes(eng):
    xyz, disp, col = RR.layered_lists(24, 130, 724)
    one = np.tile(np.array([[0.3, -0.2, 1.7]], np.float32), (4096, 1))
    two = np.array(xyz)
    d2 = np.zeros_like(disp)
    d2[np.nonzero(PR.valid_of(xyz, disp))[0][:2]] = 1.0
    holes = np.array(xyz)
    holes[3::11, 0] = np.inf
    holes[5::13, 1] = -np.inf
    holes[7::17, 2] = np.nan
    cases = [("all invalid", xyz, np.zeros_like(disp), col, 0.03), ("two valid", two, d2, col, 0.03),
             ("identical", one, None, None, 0.03), ("2^20", np.array(xyz) * F32(2.0 ** 20), disp, col, 0.03 * 2.0 ** 20),
             ("2^-20", np.array(xyz) * F32(2.0 ** -20), disp, col, 0.03 * 2.0 ** -20), ("holes", holes, disp, col, 0.03)]
    for what, p, d, c, t in cases:
        for select in (0, 1):
            w = everything(eng, p, d, c, F32(t), 64, 5, 1, select, what=what)
        if what in ("all invalid", "two valid", "identical"):
            assert int(w["stats"][7]) == 0 and not w["model"].any()
        else:
            assert int(w["stats"][7]) == 1 and int(w["stats"][6]) == 1
    assert int(PR.segment(one, None, None, 0.03, 64, 5)["stats"][1]) == 64


def test_plane_inliers_on_hand_made_models_and_its_refusals(eng):
    xyz, disp, col = RR.layered_lists(24, 130, 724)
    r = F32(1.0 / np.sqrt(2.0))
    for model, t in (([0, 0, -1, 2], 0.05), ([0, 0, 1, -1.2], 0.02), ([r, 0, -r, 1.0], 0.3), ([0.6, 0.8, 0, 0], 0.1), ([0, 0, 1.0004, -2], 0.05)):
        for select in (0, 1):
            want = PR.classify(xyz, disp, col, F32(model), t, select)
            for fn in (host, device):
                same(fn(eng, xyz, disp, col, t, 0, 0, 0, select, model=model), want, (model, fn.__name__))
    L = _lib.load()
    n = 100
    X = np.array(xyz[:n])
    inl, idx = np.full(n, MARK_B, np.uint8), np.full(n, MARK_I, np.uint32)
    ni, ns = C.c_int64(MARK_N), C.c_int64(MARK_N)
    mk = lambda *m: np.array(m, np.float32)
    good = mk(0, 0, 1, 0)
    h = eng._h
    out = (inl.ctypes.data, None, None, None, idx.ctypes.data, C.byref(ni), C.byref(ns))
    bad = [(h, X.ctypes.data, None, None, n, m.ctypes.data, 0.05, 0) + out
           for m in (mk(0, 0, 2, 0), mk(0, 0, np.nan, 0), mk(0, 0, 1, np.inf), mk(0, 0, 0, 0), mk(0, 0, 1.002, 0))]
    bad += [(h, X.ctypes.data, None, None, n, good.ctypes.data, t, 0) + out for t in (0.0, -1.0, float("nan"), float("inf"), 1e-45, 1e-39)]
    bad += [(h, X.ctypes.data, None, None, n, good.ctypes.data, 0.05, s) + out for s in (2, -1)]
    bad += [(h, X.ctypes.data, None, None, n, None, 0.05, 0) + out, (h, None, None, None, n, good.ctypes.data, 0.05, 0) + out,
            (h, X.ctypes.data, None, None, -1, good.ctypes.data, 0.05, 0) + out,
            (h, X.ctypes.data, None, None, n, good.ctypes.data, 0.05, 0, inl.ctypes.data, None, None, idx.ctypes.data, None, C.byref(ni), C.byref(ns)),
            (h, X.ctypes.data, None, None, n, good.ctypes.data, 0.05, 0, None, None, None, None, None, None, C.byref(ns))]
    for fn in (L.sgm_plane_inliers, L.sgm_plane_inliers_device):
        for args in bad:
            assert fn(*args) == -1 and b"sgm_plane_inliers" in L.sgm_last_error(), args
        assert fn(h, X.ctypes.data, None, None, 1 << 24, good.ctypes.data, 0.05, 0, *out) == -4 and b"2^24" in L.sgm_last_error()
    assert (inl == MARK_B).all() and (idx == MARK_I).all() and (ni.value, ns.value) == (MARK_N, MARK_N)


def test_refusals_leave_the_outputs_untouched_and_the_engine_usable(eng):
    L = _lib.load()
    xyz, disp, col = RR.layered_lists(24, 130, 724)
    n = 100
    X = np.array(xyz[:n])
    g = _marked(n, ALL, None)
    ni, ns = C.c_int64(MARK_N), C.c_int64(MARK_N)
    at = lambda a: None if a is None else a.ctypes.data
    out = tuple(at(g[k]) for k in ALL)
    ref = (C.byref(ni), C.byref(ns))
    h, Xp = eng._h, X.ctypes.data
    call = lambda e=h, x=Xp, c=None, n_=n, t=0.05, K=16, seed=0, refine=1, select=0, o=out, r=ref: (e, x, None, c, n_, t, K, seed, refine, select) + o + r
    bad = [call(e=None), call(x=None), call(r=(None, C.byref(ns))), call(n_=-1)]
    bad += [call(t=t) for t in (0.0, -1.0, float("nan"), float("inf"), 1e-45, 1e-39)]
    bad += [call(K=K) for K in (0, -3, 65537, 1 << 30)] + [call(refine=r) for r in (2, -1)] + [call(select=s) for s in (2, -1)]
    bad += [call(o=out[:3] + (Xp,) + out[4:])]                      # out_colors without colors_rgb
    for fn in (L.sgm_segment_plane, L.sgm_segment_plane_device):
        for args in bad:
            assert fn(*args) == -1, args                                   # SGM_ERR_INVALID_ARG
            assert b"sgm_segment_plane" in L.sgm_last_error()
        assert fn(*call(n_=1 << 24)) == -4 and b"2^24" in L.sgm_last_error()      # SGM_ERR_UNSUPPORTED: before anything is read
    assert all(np.array_equal(v, w) for v, w in zip((g[k] for k in ALL if g[k] is not None), (x for x in _marked(n, ALL, None).values() if x is not None)))
    assert (ni.value, ns.value) == (MARK_N, MARK_N)
    # n = 0 succeeds as "no plane" with nothing else written
    for fn in (L.sgm_segment_plane, L.sgm_segment_plane_device):
        ni.value = ns.value = MARK_N
        assert fn(*call(n_=0)) == 0 and (ni.value, ns.value) == (0, 0) and g["stats"].tolist() == [0] * 8 and not g["model"].any()
        assert fn(h, Xp, None, None, 0, 0.05, 16, 0, 1, 0, None, None, None, None, None, None, None, C.byref(ni), None) == 0
    assert (g["inlier"] == MARK_B).all() and (g["index"] == MARK_I).all()
    everything(eng, xyz, disp, col, 0.03, 64, 7, want=PR.want_of("l724", xyz, disp, col, 0.03, 64, 7), what="after the refusals")


def test_five_calls_give_the_same_bytes(eng):
    xyz, disp, col, t, K, seed = PR.condition_case("layered")

    def run(bits):
        runs = [bytes_of(device(eng, xyz, disp, col, t, K, seed)) for _ in range(5)]
        assert all(r == runs[0] for r in runs[1:])
        runs = [bytes_of(host(eng, xyz, disp, col, t, K, seed)) for _ in range(5)]
        assert all(r == runs[0] for r in runs[1:])
    both_forms(eng, run)


# ---- 3. history: poisoned buffers, other calls on the same engine, the stage record -------------------------------------------------
def _radius(e, i):
    xyz, disp, col = RR.case_input(i)
    r, nb, mc, o = RR.SHAPE_CASES[i][3:]
    w = RR.case_want(i)
    p, c, keep, cnt, idx, noor = e.radius_outlier_host(xyz, disp, col, r, nb, mc, o, return_counts=True, return_index=True)
    assert np.array_equal(keep, w["keep"]) and np.array_equal(cnt, w["counts"]) and np.array_equal(idx, w["index"])
    assert np.array_equal(u32(p), u32(w["points"]))


def _dbscan(e, i):
    xyz, disp = DR.case_input(i)
    w = DR.case_want(i)
    lab, core, sizes, st = e.cluster_dbscan_host(xyz, disp, *DR.SHAPE_CASES[i][3:], return_core=True, return_sizes=True)
    assert np.array_equal(lab, w["labels"]) and np.array_equal(core, w["core"]) and np.array_equal(sizes, w["sizes"]) and st.tolist() == w["stats"].tolist()


def test_a_long_lived_engine_from_poisoned_buffers():
    """plane, clustering and radius calls interleaved at changing n and K on one engine whose buffers start as 0xA5 / 0x7F"""
    e = Engine(P16)
    last = NCASE - 1

    def pl(i, fn):
        xyz, disp, col = PR.case_input(i)
        t, K, seed, refine, select = PR.SHAPE_CASES[i][3:]
        same(fn(e, xyz, disp, col, t, K, seed, refine, select), PR.case_want(i), (i, fn.__name__))
    try:
        for byte in (0xA5, 0x7F):
            e.set_option(_lib.SGM_OPT_POISON, byte)      # fills every buffer the engine owns and arms the same for new ones
            pl(last, host)
            _radius(e, 7)                                # rad_keep, cpts and rad_idx are shared with the radius filter
            pl(8, device)                                # 4097 points
            e.set_option(_lib.SGM_OPT_POISON, byte)
            _dbscan(e, 8)
            pl(18, device)                               # 4097 hypotheses on 257 points
            pl(2, host)                                  # three points
            e.trim()                                     # gives the valid list, the hypotheses and the staged outputs back
            pl(20, host)
            _radius(e, 5)
            pl(0, device)                                # one point: no plane
        e.set_option(_lib.SGM_OPT_DEBUG, OTHER)
        e.set_option(_lib.SGM_OPT_POISON, 0xA5)
        pl(last, host)
        pl(17, device)
    finally:
        e.set_option(_lib.SGM_OPT_POISON, -1)
        e.set_option(_lib.SGM_OPT_DEBUG, 0)


def test_the_profile_record_names_the_stages():
    e = Engine(P16)
    xyz, disp, col, t, K, seed = PR.condition_case("layered")
    full = {"plane_valid": 3, "plane_sample": 1, "plane_count": 1, "plane_best": 1, "plane_moments": 1, "plane_solve": 1, "plane_classify": 1,
            "plane_compact": 3, "_wall": 0}
    try:
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        for bits in (0, OTHER):
            e.set_option(_lib.SGM_OPT_DEBUG, bits)
            same(device(e, xyz, disp, col, t, K, seed), PR.want_of("layered", xyz, disp, col, t, K, seed))
            st = {n: launches for n, ms, launches in e.stage_times()}
            assert st == full and tuple(n for n, ms, k in e.stage_times() if n != "_wall") == _lib.PLANE_STAGES, st
            assert all(ms >= 0 for n, ms, k in e.stage_times())
        same(host(e, xyz, disp, col, t, K, seed, 0, 0, outs=("inlier", "model")), PR.want_of("layered", xyz, disp, col, t, K, seed, False, 0))
        st = {n: k for n, ms, k in e.stage_times()}
        assert "plane_moments" not in st and "plane_solve" not in st and st["plane_compact"] == 2, st
        host(e, xyz, disp, col, t, 0, 0, 0, 0, model=[0, 0, -1, 1.2])
        assert {n: k for n, ms, k in e.stage_times()} == {"plane_classify": 1, "plane_compact": 3, "_wall": 0}
    finally:
        e.set_option(_lib.SGM_OPT_PROFILE, 0)
        e.set_option(_lib.SGM_OPT_DEBUG, 0)


def test_the_other_cloud_calls_are_unchanged_with_plane_calls_between_them():
    e = Engine(P16)
    xyz, disp, col = VR.layered_cloud(97, 331, 9)
    lst = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)

    def plane():
        g = host(e, *lst, 0.03, 48, 4, 1, 1)
        assert g["stats"][7] == 1 and 0 < g["n_inliers"] < g["stats"][0]
        return bytes_of(g)
    first = plane()
    w = RR.cells(*lst, 0.02, 8, 12)
    p, c, keep, cnt, idx, noor = e.radius_outlier_host(*lst, 0.02, 8, 12, return_counts=True, return_index=True)
    assert np.array_equal(keep, w["keep"]) and np.array_equal(cnt, w["counts"]) and np.array_equal(idx, w["index"]) and noor == w["n_out_of_range"]
    assert np.array_equal(u32(p), u32(w["points"])) and np.array_equal(c, w["colors"])
    assert plane() == first
    w = DR.cells(lst[0], lst[1], 0.02, 6)
    lab, core, sizes, st = e.cluster_dbscan_host(lst[0], lst[1], 0.02, 6, return_core=True, return_sizes=True)
    assert np.array_equal(lab, w["labels"]) and np.array_equal(sizes, w["sizes"]) and st.tolist() == w["stats"].tolist()
    assert plane() == first
    w = VR.voxel_downsample(*lst, 0.05, (0, 0, 0), 2)
    p, c, k, noor = e.voxel_downsample_host(*lst, 0.05, (0, 0, 0), 2, return_counts=True)
    assert np.array_equal(u32(p), u32(w["points"])) and np.array_equal(c, w["colors"]) and np.array_equal(k, w["counts"])
    pts, cols = e.compact_points_host(xyz, disp, col)
    ok = np.isfinite(lst[0][:, 0]) & (lst[1] > 0)
    assert np.array_equal(u32(pts), u32(lst[0][ok])) and np.array_equal(cols, lst[2][ok])
    assert plane() == first
    same(host(e, *lst, 0.03, 48, 4, 1, 1), PR.segment(*lst, 0.03, 48, 4, True, 1), "97 x 331")


# ---- 4. the Python surface -------------------------------------------------------------------------------------------------------------
def test_segment_plane_on_numpy_input_and_on_tensors():
    import torch
    xyz, disp, col, t, K, seed = PR.condition_case("layered")
    img, dmap, cimg = np.array(xyz).reshape(48, 320, 3), np.array(disp).reshape(48, 320), np.array(col).reshape(48, 320, 3)
    want = PR.want_of("layered", xyz, disp, col, t, K, seed)
    inv = PR.want_of("layered", xyz, disp, col, t, K, seed, True, 1)
    stats = dict(zip(PR.STATS, (int(x) for x in want["stats"])))
    model, mask = sgm.segment_plane(img, None, dmap, t, num_iterations=K, seed=seed)
    assert model.dtype == np.float32 and np.array_equal(u32(model), u32(want["model"]))
    assert mask.shape == (48, 320) and mask.dtype == np.uint8 and np.array_equal(mask.reshape(-1), want["inlier"])
    model, mask, pts, cols, idx, dist, st = sgm.segment_plane(img, cimg, dmap, t, num_iterations=K, seed=seed, return_points=True,
                                                               return_index=True, return_distances=True, return_stats=True)
    assert st == stats and np.array_equal(u32(pts), u32(want["points"])) and np.array_equal(cols, want["colors"])
    assert np.array_equal(idx, want["index"]) and dist.shape == (48, 320) and np.array_equal(u32(dist.reshape(-1)), u32(want["distance"]))
    # inverted: the mask of the valid points off the plane, into cluster_dbscan and valid_points
    model, off, pts, cols = sgm.segment_plane(img, cimg, dmap, t, num_iterations=K, seed=seed, invert=True, return_points=True)
    assert np.array_equal(off.reshape(-1), inv["selected"]) and np.array_equal(u32(pts), u32(inv["points"])) and np.array_equal(cols, inv["colors"])
    p2, c2 = sgm.valid_points(img, cimg, dmap, confidence=off, min_confidence=1)
    assert np.array_equal(u32(p2), u32(inv["points"])) and np.array_equal(c2, inv["colors"])
    lab = sgm.cluster_dbscan(img, dmap, 0.05, 4, confidence=off, min_confidence=1)
    w = DR.cells(np.array(xyz), np.where(inv["selected"] > 0, disp, F32(0)), 0.05, 4)
    assert np.array_equal(lab.reshape(-1), w["labels"]) and (lab.reshape(-1)[want["inlier"] > 0] == -1).all()
    # the next plane: the previous inverted mask as confidence
    w2 = PR.segment(xyz, np.where(inv["selected"] > 0, disp, F32(0)), None, t, K, seed)
    m2, mask2 = sgm.segment_plane(img, None, dmap, t, num_iterations=K, seed=seed, confidence=off, min_confidence=1)
    assert np.array_equal(u32(m2), u32(w2["model"])) and np.array_equal(mask2.reshape(-1), w2["inlier"]) and not (mask2 & mask).any()
    # plane_inliers with the model found
    m = sgm.plane_inliers(img, None, dmap, model, t)
    assert np.array_equal(m.reshape(-1), want["inlier"])
    m, d = sgm.plane_inliers(img, None, dmap, model, t, invert=True, return_distances=True)
    assert np.array_equal(m.reshape(-1), inv["selected"]) and np.array_equal(u32(d.reshape(-1)), u32(want["distance"]))
    # a list
    lst = np.array(xyz)[PR.valid_of(xyz, disp)]
    w3 = PR.segment(lst, None, None, t, 100, 3)
    m3, k3, i3 = sgm.segment_plane(lst, None, None, t, num_iterations=100, seed=3, return_index=True)
    assert k3.shape == (lst.shape[0],) and np.array_equal(u32(m3), u32(w3["model"])) and np.array_equal(k3, w3["inlier"]) and np.array_equal(i3, w3["index"])
    # HIP tensors stay on the device
    ti, td, tc = torch.from_numpy(img).cuda(), torch.from_numpy(dmap).cuda(), torch.from_numpy(cimg).cuda()
    model, tm, tp, tcol, tidx, tdist, st = sgm.segment_plane(ti, tc, td, t, num_iterations=K, seed=seed, return_points=True, return_index=True,
                                                            return_distances=True, return_stats=True)
    assert tm.is_cuda and tm.shape == (48, 320) and tm.dtype == torch.uint8 and st == stats and np.array_equal(u32(model), u32(want["model"]))
    assert np.array_equal(tm.cpu().numpy().reshape(-1), want["inlier"]) and np.array_equal(u32(tp.cpu().numpy()), u32(want["points"]))
    assert np.array_equal(tcol.cpu().numpy(), want["colors"]) and np.array_equal(tidx.cpu().numpy().view(np.uint32), want["index"])
    assert np.array_equal(u32(tdist.cpu().numpy().reshape(-1)), u32(want["distance"]))
    model, toff = sgm.segment_plane(ti, None, td, t, num_iterations=K, seed=seed, invert=True)
    assert toff.is_cuda and np.array_equal(toff.cpu().numpy().reshape(-1), inv["selected"])
    tl = sgm.cluster_dbscan(ti, td, 0.05, 4, confidence=toff, min_confidence=1)
    assert np.array_equal(tl.cpu().numpy().reshape(-1), w["labels"])
    tm2 = sgm.plane_inliers(ti, None, td, model, t, invert=True)
    assert np.array_equal(tm2.cpu().numpy().reshape(-1), inv["selected"])
    with pytest.raises(sgm.error, match="float32 and on the GPU"):
        sgm.segment_plane(torch.from_numpy(img), None, td, t)
    with pytest.raises(sgm.error, match="uint8 tensor"):
        sgm.segment_plane(ti, cimg, td, t)


def test_a_270_x_480_frame_from_the_pipeline():
    """270 x 480 through sgm_pipeline_device, then the plane of its cloud against the reference, and the objects off it"""
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
    ok = np.isfinite(xyz).all(axis=2) & (disp > 0)
    z = xyz[..., 2][ok]
    t = float(F32(0.02 * float(np.median(np.abs(z)))))
    want = PR.segment(xyz.reshape(-1, 3), disp.reshape(-1), None, t, 32, 1)
    assert int(want["stats"][7]) == 1 and want["n_inliers"] >= 3
    model, mask, dist, st = sgm.segment_plane(xyz, None, disp, t, num_iterations=32, seed=1, return_distances=True, return_stats=True)
    assert np.array_equal(u32(model), u32(want["model"])) and np.array_equal(mask.reshape(-1), want["inlier"])
    assert np.array_equal(u32(dist.reshape(-1)), u32(want["distance"])) and st == dict(zip(PR.STATS, (int(x) for x in want["stats"])))
    tm, tmask = sgm.segment_plane(dx, None, df, t, num_iterations=32, seed=1)
    assert np.array_equal(u32(tm), u32(want["model"])) and np.array_equal(tmask.cpu().numpy().reshape(-1), want["inlier"])


# ---- 5. full size ----------------------------------------------------------------------------------------------------------------------
def test_a_full_size_lattice_with_every_seventh_point_lifted():
    """2160 x 4096 points at spacing 0.25 in the plane Z = 2, every 7th lifted by 0.5, K = 64, t = 0.01: whatever three points a
    hypothesis draws, the only plane with more than a seventh of the points is Z = 2, so the model is exactly (0, 0, -1, 2), the
    inliers are the points that were not lifted, their distances are 0 and those of the others -0.5; under both counting forms."""
    import torch
    H, W = 2160, 4096
    n = H * W
    e = Engine(P16)
    y, x = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    up = (torch.arange(n, device="cuda") % 7) == 6
    z = torch.where(up, torch.tensor(2.5, device="cuda"), torch.tensor(2.0, device="cuda")).reshape(H, W)
    dx = torch.stack([x * 0.25 - 3.0, y * 0.25 - 1.0, z], dim=2).reshape(n, 3).contiguous()
    del x, y, z
    inl = torch.full((n,), MARK_B, dtype=torch.uint8, device="cuda")
    dist = torch.empty(n, dtype=torch.float32, device="cuda")
    idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    before = dx.clone()
    n_up = int(up.sum())
    first = None
    try:
        for bits in (0, OTHER):
            e.set_option(_lib.SGM_OPT_DEBUG, bits)
            torch.cuda.synchronize()
            model, st, ni, ns = e.segment_plane_device(dx.data_ptr(), None, None, n, 0.01, 64, 0, True, 1, inl.data_ptr(), dist.data_ptr(), None, None,
                                                       idx.data_ptr())
            assert np.array_equal(u32(model), u32(F32([0, 0, -1, 2]))), model
            assert (ni, ns) == (n - n_up, n_up) and st[0] == n and st[3] == n - n_up and st[6] == 1 and st[7] == 1, (ni, ns, st)
            assert st[4] + st[5] == n - n_up and st[5] > 0                  # the lattice is wider than +-16384 t: some inliers do not vote
            assert bool((inl == (~up).to(torch.uint8)).all()) and bool((dist == torch.where(up, -0.5, 0.0)).all())
            assert bool((idx[:ns].to(torch.int64) == torch.nonzero(up).reshape(-1)).all()) and bool((idx[ns:] == -1).all())
            first = first or st.tolist()
            assert st.tolist() == first
    finally:
        e.set_option(_lib.SGM_OPT_DEBUG, 0)
    assert bool((dx == before).all())


# ---- 6. guarded buffers -------------------------------------------------------------------------------------------------------------------
def test_the_cases_with_every_buffer_guarded():
    """(the same cases ran in the plain mode above)"""
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "plane_guard_child.py")], capture_output=True, text=True, env=env,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"PLANE_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) >= 8, tail
