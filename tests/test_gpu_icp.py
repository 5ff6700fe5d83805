"""Rigid registration on the device (needs an MI355X): sgm_register_icp, sgm_register_icp_device, sgm_evaluate_registration,
sgm_evaluate_registration_device, sgm_transform_points, sgm_transform_points_device, the Engine methods over them,
sgm.registration_icp, sgm.evaluate_registration, sgm.transform_points.

Yardstick: tests/icp_ref.py -- the definition of include/sgm_hip_icp.h in numpy -- bit for bit: the transformation, fitness, rmse and
the history as uint64, the squared distances as uint32, the correspondences and the eight statistics exactly, through both entries
and under both estimations.  Every output is pre-filled with a marker, the history rows past the last evaluation must keep it, and
every input is checked unmodified."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import covariance_ref as CR
import dbscan_ref as DR
import icp_ref as IR
import parity_util as U
import plane_ref as PR
import radius_ref as RR
import statistical_ref as SR
import voxel_ref as VR
import stereo_reconstruction_cv_amd as sgm
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = dict(numDisparities=16)
MARK_F, MARK_I, MARK_S, MARK_D = 0xC2F6E979, -0x21524111, 0xABCDEF0123456789, 0xC0FFEE0012345678
ALL = ("T", "fitness", "rmse", "corr", "d2", "history", "stats")
F32 = np.float32
EYE = np.eye(4)


@pytest.fixture(scope="module")
def eng():
    return Engine(P16)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _marked(ns, maxit, outs):
    m = max(ns, 1)
    dbl = lambda k: np.full(k, MARK_D, np.uint64).view(np.float64)
    return dict(T=dbl(16) if "T" in outs else None, fitness=dbl(1) if "fitness" in outs else None, rmse=dbl(1) if "rmse" in outs else None,
                corr=np.full(m, MARK_I, np.int32) if "corr" in outs else None,
                d2=np.full(m, MARK_F, np.uint32).view(np.float32) if "d2" in outs else None,
                history=dbl(2 * (maxit + 3)) if "history" in outs else None,
                stats=np.full(8, MARK_S, np.uint64) if "stats" in outs else None)


def _args(src, ds, tgt, dt, tn, origin, T0):
    src = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
    tgt = np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
    ds = None if ds is None else np.ascontiguousarray(ds, np.float32)
    dt = None if dt is None else np.ascontiguousarray(dt, np.float32)
    tn = None if tn is None else np.ascontiguousarray(tn, np.float32)
    return src, ds, tgt, dt, tn, np.ascontiguousarray(origin, np.float32), np.ascontiguousarray(EYE if T0 is None else T0, np.float64).reshape(16)


def call(e, entry, src, ds, tgt, dt, tn, r, est=1, maxit=30, T0=None, origin=(0, 0, 0), rf=1e-6, rr=1e-6, outs=ALL, evaluate=False, rc_want=0):
    """sgm_register_icp (or, with evaluate, sgm_evaluate_registration) through the host or the device entry on marked outputs: a dict
    of whole arrays (None where not asked for)"""
    src, ds, tgt, dt, tn, org, T0 = _args(src, ds, tgt, dt, tn, origin, T0)
    ns, nt = src.shape[0], tgt.shape[0]
    before = [None if a is None else a.copy() for a in (src, ds, tgt, dt, tn, org, T0)]
    g = _marked(ns, maxit, outs)
    at = lambda a: None if a is None else a.ctypes.data
    L = _lib.load()
    if entry == "host":
        p = [at(src), at(ds), ns, at(tgt), at(dt), at(tn), nt]
        pc, pd = at(g["corr"]), at(g["d2"])
    else:
        import torch
        dev = torch.device("cuda", e.device)
        up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
        t_in = [up(a) for a in (src, ds, tgt, dt, tn)]
        t_corr, t_d2 = up(g["corr"]), up(None if g["d2"] is None else g["d2"].view(np.int32))
        ptr = lambda x: None if x is None else x.data_ptr()
        p = [ptr(t_in[0]), ptr(t_in[1]), ns, ptr(t_in[2]), ptr(t_in[3]), ptr(t_in[4]), nt]
        pc, pd = ptr(t_corr), ptr(t_d2)
        torch.cuda.synchronize()
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    if evaluate:
        fn = L.sgm_evaluate_registration if entry == "host" else L.sgm_evaluate_registration_device
        rc = fn(e._h, p[0], p[1], p[2], p[3], p[4], p[6], float(r), at(org), at(T0), dp(g["fitness"]), dp(g["rmse"]), pc, pd, at(g["stats"]))
    else:
        fn = L.sgm_register_icp if entry == "host" else L.sgm_register_icp_device
        rc = fn(e._h, *p, float(r), at(org), at(T0), int(est), int(maxit), float(rf), float(rr), at(g["T"]), dp(g["fitness"]), dp(g["rmse"]),
                pc, pd, at(g["history"]), at(g["stats"]))
    assert rc == rc_want, (rc, _lib.last_error())
    if entry != "host":
        e.synchronize()
        for a, t in zip((src, ds, tgt, dt, tn), t_in):
            assert a is None or np.array_equal(t.cpu().numpy(), a, equal_nan=True)
        if t_corr is not None:
            g["corr"] = t_corr.cpu().numpy()
        if t_d2 is not None:
            g["d2"] = t_d2.cpu().numpy().view(np.float32)
    for a, b in zip((src, ds, tgt, dt, tn, org, T0), before):
        assert a is None or np.array_equal(a, b, equal_nan=True)
    return dict(g, ns=ns, maxit=maxit)


def untouched(g):
    for k, mark in (("T", MARK_D), ("fitness", MARK_D), ("rmse", MARK_D), ("history", MARK_D), ("stats", MARK_S)):
        assert g[k] is None or (g[k].view(np.uint64) == mark).all(), k
    assert g["corr"] is None or (g["corr"] == MARK_I).all()
    assert g["d2"] is None or (u32(g["d2"]) == MARK_F).all()


def same(g, w, what="", evaluate=False):
    """the marked outputs of a call against the reference's dict, bit for bit"""
    ns = g["ns"]
    if g["stats"] is not None:
        assert g["stats"].tolist() == w["stats"].tolist(), (what, g["stats"], w["stats"])
    if g["T"] is not None:
        assert u64(g["T"]).tolist() == u64(w["T"]).reshape(-1).tolist(), (what, g["T"], w["T"])
    for k in ("fitness", "rmse"):
        assert g[k] is None or u64(g[k])[0] == u64([w[k]])[0], (what, k, g[k], w[k])
    if g["corr"] is not None:
        assert np.array_equal(g["corr"][:ns], w["corr"]), what
        assert (g["corr"][ns:] == MARK_I).all()
    if g["d2"] is not None:
        assert np.array_equal(u32(g["d2"][:ns]), u32(w["d2"])), what
        assert (u32(g["d2"][ns:]) == MARK_F).all()
    if g["history"] is not None and not evaluate:
        rows = w["history"].shape[0]
        assert rows <= g["maxit"] + 1
        assert u64(g["history"][:2 * rows]).tolist() == u64(w["history"]).reshape(-1).tolist(), what
        assert (g["history"][2 * rows:].view(np.uint64) == MARK_D).all(), what


def bytes_of(g):
    return b"".join(np.ascontiguousarray(g[k]).tobytes() for k in ALL if g[k] is not None)


def ref(key, *a, **k):
    return IR.shared(("gpu",) + key, lambda: IR.register(*a, **k))


# ---- 1. the shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", (0, 1))
@pytest.mark.parametrize("with_disp", (True, False))
@pytest.mark.parametrize("i", range(len(IR.SHAPE_CASES)))
def test_shapes_through_both_entries(eng, i, with_disp, est):
    src, ds, tgt, dt, tn = IR.case_input(i)
    w = IR.case_want(i, with_disp, est)
    for entry in ("host", "device"):
        g = call(eng, entry, src, ds if with_disp else None, tgt, dt if with_disp else None, tn, IR.R_CASE, est, IR.SHAPE_ITERATIONS)
        same(g, w, (IR.SHAPE_CASES[i], with_disp, est, entry))


def test_each_optional_output_null_in_turn(eng):
    i = IR.SHAPE_CASES.index((257, 300))
    src, ds, tgt, dt, tn = IR.case_input(i)
    w = IR.case_want(i, True, 1)
    for entry in ("host", "device"):
        for drop in ALL:
            same(call(eng, entry, src, ds, tgt, dt, tn, IR.R_CASE, 1, IR.SHAPE_ITERATIONS, outs=tuple(k for k in ALL if k != drop)), w, (entry, drop))
        same(call(eng, entry, src, ds, tgt, dt, tn, IR.R_CASE, 1, IR.SHAPE_ITERATIONS, outs=("T",)), w, entry)
        call(eng, entry, src, ds, tgt, dt, tn, IR.R_CASE, 1, IR.SHAPE_ITERATIONS, outs=())


def test_more_than_1024_blocks_of_partial_sums(eng):
    """266 240 source points: k_icp_reduce loops.  The partner of lattice point i is point i, so the reference needs only its terms
    and its tree; one iteration from there is the reference's solve of those sums."""
    src, tgt, nrm, r, corr = IR.big_lattice()
    assert src.shape[0] > 1024 * 256
    cl = IR.Clouds(src, None, tgt, None, nrm, r)
    for est in (0, 1):
        ev = IR.evaluate(cl, EYE, est, known_corr=corr)
        g = call(eng, "device", src, None, tgt, None, nrm, r, est, 0)
        assert np.array_equal(g["corr"], corr) and np.array_equal(u32(g["d2"]), u32(ev["d2"]))
        assert u64(g["fitness"])[0] == u64([ev["fitness"]])[0] and u64(g["rmse"])[0] == u64([ev["rmse"]])[0]
        assert g["stats"].tolist() == [src.shape[0], src.shape[0], 0, 0, src.shape[0], 0, 0, IR.MAX_ITER]
        T1, st = IR.solve_update(ev["sums"], EYE)
        assert st == 0
        g = call(eng, "device", src, None, tgt, None, nrm, r, est, 1, outs=("T", "history", "stats"))
        assert u64(g["T"]).tolist() == u64(T1).reshape(-1).tolist(), est
        assert u64(g["history"][:2]).tolist() == u64([ev["fitness"], ev["rmse"]]).tolist() and int(g["stats"][3]) == 1


# ---- 2. the edges of the correspondence ------------------------------------------------------------------------------------------------
def both(eng, key, src, ds, tgt, dt, tn, r, est=0, maxit=0, **k):
    w = ref(key, src, ds, tgt, dt, tn, r, origin=k.get("origin", (0.0, 0.0, 0.0)), T0=k.get("T0"), estimation=est, max_iteration=maxit,
            how=k.pop("how", "auto"))
    for entry in ("host", "device"):
        same(call(eng, entry, src, ds, tgt, dt, tn, r, est, maxit, **k), w, (key, entry))
    return w


def test_partners_across_every_face_edge_and_corner_of_a_cell(eng):
    for origin in ((0.0, 0.0, 0.0), (0.37, -1.2, 0.05)):
        xyz, dirs = RR.face_pairs(0.05, origin)
        src, tgt = np.ascontiguousarray(xyz[0::2]), np.ascontiguousarray(xyz[1::2][::-1])
        w = both(eng, ("faces", origin), src, None, tgt, None, None, 0.05, origin=origin, how="brute")
        assert w["corr"].tolist() == list(range(25, -1, -1)) and len(dirs) == 26
        _, _, gs = RR.classify(src, None, 0.05, origin)
        _, _, gt = RR.classify(tgt[::-1], None, 0.05, origin)
        assert sorted(map(tuple, (gt - gs).tolist())) == sorted(map(tuple, dirs.tolist()))      # the pairs do straddle all 26


def test_ties_the_radius_identical_points_and_a_full_cell(eng):
    src, _, tgt, _, _, r = IR.condition_case("tie")
    w = both(eng, ("tie",), src, None, tgt, None, None, r)
    assert w["corr"].tolist() == [2 * k for k in range(300)]
    # exactly at r and one ulp beyond
    r = F32(0.25)
    k = np.arange(200, dtype=F32)
    src = np.stack([np.zeros(200, F32), k * F32(4.0), np.zeros(200, F32)], axis=1)
    tgt = src.copy()
    tgt[:, 0] = np.where(np.arange(200) % 2 == 0, r, np.nextafter(r, F32(1)))
    w = both(eng, ("at r",), src, None, tgt, None, None, r, how="brute")
    assert w["corr"].tolist() == [j if j % 2 == 0 else -1 for j in range(200)]
    # 4096 identical target points: the lowest index; and a cell of 4097
    src = np.array([[0.5, 0.5, 0.5], [0.51, 0.5, 0.5]], F32)
    tgt = np.tile(np.array([[0.505, 0.5, 0.5]], F32), (4096, 1))
    w = both(eng, ("identical",), src, None, tgt, None, None, 0.1, how="brute")
    assert w["corr"].tolist() == [0, 0]
    rng = np.random.default_rng(5)
    tgt = (np.array([0.5, 0.5, 0.5], F32) + (rng.random((4097, 3)) * 0.01).astype(F32)).astype(F32)
    src = (np.array([0.5, 0.5, 0.5], F32) + (rng.random((100, 3)) * 0.01).astype(F32)).astype(F32)
    assert len(set(map(tuple, RR.classify(tgt, None, 0.1, (0, 0, 0))[2].tolist()))) == 1
    both(eng, ("full cell",), src, None, tgt, None, None, 0.1, how="brute")


def test_inputs_with_nothing_to_use(eng):
    src, ds, tgt, dt, tn = IR.case_input(IR.SHAPE_CASES.index((257, 300)))
    nan = np.full_like(src, np.nan)
    far = np.array(src) + F32(1.0e7)
    w = both(eng, ("src invalid",), nan, None, tgt, dt, tn, IR.R_CASE, 1, 3)
    assert w["stats"].tolist()[0] == 0 and int(w["stats"][7]) == IR.TOO_FEW
    w = both(eng, ("src far",), far, None, tgt, dt, tn, IR.R_CASE, 1, 3)
    assert int(w["stats"][5]) == int(w["stats"][0]) > 0 and int(w["stats"][7]) == IR.TOO_FEW
    w = both(eng, ("tgt invalid",), src, ds, np.full_like(tgt, np.inf), None, tn, IR.R_CASE, 1, 3)
    assert w["stats"].tolist()[1:3] == [0, 0] and (w["corr"] == -1).all()
    w = both(eng, ("tgt far",), src, ds, np.where(np.isfinite(tgt), np.array(tgt) + F32(1.0e7), tgt), dt, tn, IR.R_CASE, 1, 3)
    assert int(w["stats"][1]) == 0 and int(w["stats"][2]) > 0
    both(eng, ("no tgt",), src, ds, np.zeros((0, 3), F32), None, None, IR.R_CASE, 0, 3)
    T0 = EYE.copy()
    T0[:3, 3] = (1.0e6, 0.0, 0.0)                    # the transformation itself takes the source out of range
    w = both(eng, ("T0 far",), src, ds, tgt, dt, tn, IR.R_CASE, 1, 3, T0=T0)
    assert int(w["stats"][5]) == int(w["stats"][0]) > 0
    # an empty source: nothing runs
    for entry in ("host", "device"):
        g = call(eng, entry, np.zeros((0, 3), F32), None, tgt, dt, tn, IR.R_CASE, 1, 3, T0=T0)
        assert g["stats"].tolist() == [0, 0, 0, 0, 0, 0, 0, 2] and u64(g["T"]).tolist() == u64(T0).reshape(-1).tolist()
        assert g["fitness"][0] == 0 and g["rmse"][0] == 0 and g["history"][:2].tolist() == [0, 0] and (g["history"][2:].view(np.uint64) == MARK_D).all()


def test_negative_coordinates_an_origin_and_the_scales(eng):
    src, tgt, tn, _ = IR.recovery_case(600, 47)
    shift = np.array([-3.0, -2.0, -5.0], F32)
    both(eng, ("negative",), src + shift, None, tgt + shift, None, tn, IR.R_CASE, 1, 4, origin=(-0.013, 0.4, -7.0))
    for name, s in (("2^20", 2.0 ** 20), ("2^-20", 2.0 ** -20)):
        S = F32(s)
        for est in (0, 1):
            w = both(eng, (name, est), src * S, None, tgt * S, None, tn, float(F32(IR.R_CASE) * S), est, 4)
            assert int(w["stats"][4]) > 300, (name, w["stats"])


def test_the_plane_the_corner_the_iteration_counts_and_every_status(eng):
    src, _, tgt, _, tn, r = IR.condition_case("plane")
    w = both(eng, ("plane",), src, None, tgt, None, tn, r, 1, 30)
    assert int(w["stats"][7]) == IR.DEGENERATE
    src, _, tgt, _, tn, r = IR.condition_case("corner")
    seen = {IR.DEGENERATE}
    for est in (0, 1):
        seen.add(int(both(eng, ("corner", est), src, None, tgt, None, tn, r, est, 30)["stats"][7]))
    src, tgt, tn, truth = IR.recovery_case()
    for maxit in (0, 1, 5, 30):
        for est in (0, 1):
            w = both(eng, ("recovery", maxit, est), src, None, tgt, None, tn, IR.R_CASE, est, maxit)
            seen.add(int(w["stats"][7]))
    seen.add(int(both(eng, ("few",), src[:5], None, tgt, None, tn, IR.R_CASE, 1, 30)["stats"][7]))
    assert seen == {IR.CONVERGED, IR.MAX_ITER, IR.TOO_FEW, IR.DEGENERATE}
    # the evaluation entries equal the call with no iterations
    T0 = IR.rigid((0, 1, 0), 1.0, (0.01, 0.0, 0.0))
    w = ref(("recovery eval",), src, None, tgt, None, tn, IR.R_CASE, T0=T0, estimation=0, max_iteration=0)
    for entry in ("host", "device"):
        same(call(eng, entry, src, None, tgt, None, None, IR.R_CASE, T0=T0, evaluate=True, outs=("fitness", "rmse", "corr", "d2", "stats")),
             w, entry, evaluate=True)


def test_five_calls_give_the_same_bytes(eng):
    src, ds, tgt, dt, tn, r = IR.condition_case("layered")
    for entry in ("host", "device"):
        runs = [bytes_of(call(eng, entry, src, ds, tgt, dt, tn, r, 1, 6)) for _ in range(5)]
        assert all(x == runs[0] for x in runs[1:])
    same(call(eng, "device", src, ds, tgt, dt, tn, r, 1, 6), ref(("layered", 6), src, ds, tgt, dt, tn, r, estimation=1, max_iteration=6))


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


def _statistical(e, i):
    xyz, disp, col = SR.case_input(i)
    k, ratio, r, o = SR.SHAPE_CASES[i][3:]
    w = SR.case_want(i)
    p, c, keep, mean, idx, st = e.statistical_outlier_host(xyz, disp, col, k, ratio, r, o, return_distances=True)
    assert np.array_equal(keep, w["keep"]) and np.array_equal(u32(mean), u32(w["mean"])) and st.tolist() == w["stats"].tolist()


def _covariance(e, i):
    xyz, disp = CR.case_input(i)
    w = CR.case_want(i)
    nrm, curv, cnt, st = e.covariance_normals_host(xyz, disp, *CR.SHAPE_CASES[i][3:], return_curvature=True, return_counts=True)
    assert np.array_equal(u32(nrm), u32(w["normals"])) and np.array_equal(cnt, w["counts"]) and st.tolist() == w["stats"].tolist()


def _plane(e, i):
    xyz, disp, col = PR.case_input(i)
    t, K, seed, refine, select = PR.SHAPE_CASES[i][3:]
    w = PR.case_want(i)
    model, inl, dist, p, c, idx, st, ni = e.segment_plane_host(xyz, disp, col, t, K, seed, refine, select, True, True, True)
    assert np.array_equal(u32(model), u32(w["model"])) and np.array_equal(inl, w["inlier"]) and st.tolist() == w["stats"].tolist()


def test_a_long_lived_engine_from_poisoned_buffers():
    """registration, radius, covariance, statistical, clustering and plane calls interleaved at changing sizes on one engine whose buffers start as 0xA5 / 0x7F"""
    e = Engine(P16)

    def icp(ns, nt, entry, est=1, with_disp=True):
        i = IR.SHAPE_CASES.index((ns, nt))
        src, ds, tgt, dt, tn = IR.case_input(i)
        same(call(e, entry, src, ds if with_disp else None, tgt, dt if with_disp else None, tn, IR.R_CASE, est, IR.SHAPE_ITERATIONS),
             IR.case_want(i, with_disp, est), (ns, nt, entry))
    try:
        for byte in (0xA5, 0x7F):
            e.set_option(_lib.SGM_OPT_POISON, byte)      # fills every buffer the engine owns and arms the same for new ones
            icp(1000, 5000, "host")
            _radius(e, 7)                                # the table, the records and rad_keep are shared with the radius filter
            icp(257, 300, "device", 0)
            _covariance(e, 6)                            # ... and with the covariance normals and the statistical filter
            icp(255, 5000, "host", 0)
            _statistical(e, 7)
            icp(64, 300, "device", 1, False)
            e.set_option(_lib.SGM_OPT_POISON, byte)
            _dbscan(e, 8)
            icp(1000, 300, "device")
            _plane(e, len(PR.SHAPE_CASES) - 1)
            icp(1, 5000, "host", 1, False)
            e.trim()                                     # gives the correspondences, the partial sums and the staged target back
            icp(256, 1, "host")
            _radius(e, 5)
            icp(65, 5000, "device", 0, False)
    finally:
        e.set_option(_lib.SGM_OPT_POISON, -1)


def test_the_profile_record_names_the_stages():
    e = Engine(P16)
    src, ds, tgt, dt, tn, r = IR.condition_case("layered")
    full = {n: 1 for n in _lib.ICP_STAGES}
    full["_wall"] = 0
    try:
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        for maxit in (0, 3):
            same(call(e, "device", src, ds, tgt, dt, tn, r, 1, maxit), ref(("layered", maxit), src, ds, tgt, dt, tn, r, estimation=1, max_iteration=maxit))
            st = {n: launches for n, ms, launches in e.stage_times()}
            assert st == full and tuple(n for n, ms, k in e.stage_times() if n != "_wall") == _lib.ICP_STAGES, st
            assert all(ms >= 0 for n, ms, k in e.stage_times())
        call(e, "host", src, ds, np.zeros((0, 3), F32), None, None, r, 0, 2)
        assert tuple(n for n, ms, k in e.stage_times() if n != "_wall") == _lib.ICP_STAGES[5:]
    finally:
        e.set_option(_lib.SGM_OPT_PROFILE, 0)


def test_the_other_cloud_calls_are_unchanged_with_icp_calls_between_them():
    e = Engine(P16)
    xyz, disp, col = VR.layered_cloud(97, 331, 9)
    lst = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)
    src, ds, tgt, dt, tn, r = IR.condition_case("layered")

    def icp():
        g = call(e, "host", src, ds, tgt, dt, tn, r, 1, 4)
        assert g["stats"][4] > 100
        return bytes_of(g)

    def others():
        out = []
        p, c, keep, cnt, idx, noor = e.radius_outlier_host(*lst, 0.02, 8, 12, return_counts=True, return_index=True)
        out += [keep, cnt, idx, p, c]
        nrm, curv, k, st = e.covariance_normals_host(lst[0], lst[1], 0.04, return_curvature=True, return_counts=True)
        out += [nrm, curv, k, st]
        p, c, keep, mean, idx, st = e.statistical_outlier_host(*lst, 8, 1.0, 0.03, return_distances=True, return_index=True)
        out += [keep, mean, idx, st, p, c]
        lab, core, sizes, st = e.cluster_dbscan_host(lst[0], lst[1], 0.02, 6, return_core=True, return_sizes=True)
        out += [lab, core, sizes, st]
        model, inl, dist, p, c, idx, st, ni = e.segment_plane_host(*lst, 0.03, 48, 4, True, 1, True, True, True)
        out += [model, inl, dist, p, c, idx, st]
        return b"".join(np.ascontiguousarray(a).tobytes() for a in out)
    before = others()
    first = icp()
    assert others() == before
    w = RR.cells(*lst, 0.02, 8, 12)
    p, c, keep, cnt, idx, noor = e.radius_outlier_host(*lst, 0.02, 8, 12, return_counts=True, return_index=True)
    assert np.array_equal(keep, w["keep"]) and np.array_equal(cnt, w["counts"]) and np.array_equal(idx, w["index"])
    assert icp() == first
    w = DR.cells(lst[0], lst[1], 0.02, 6)
    lab, core, sizes, st = e.cluster_dbscan_host(lst[0], lst[1], 0.02, 6, return_core=True, return_sizes=True)
    assert np.array_equal(lab, w["labels"]) and np.array_equal(sizes, w["sizes"]) and st.tolist() == w["stats"].tolist()
    assert icp() == first and others() == before


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched_and_the_engine_usable(eng):
    i = IR.SHAPE_CASES.index((257, 300))
    src, ds, tgt, dt, tn = IR.case_input(i)
    bad_T = []
    for k, v in ((0, np.nan), (7, np.inf), (12, 1.0), (15, 2.0), (15, 0.0), (13, -1e-300)):
        T = EYE.reshape(16).copy()
        T[k] = v
        bad_T.append(T)
    for entry in ("host", "device"):
        for T in bad_T:
            untouched(call(eng, entry, src, ds, tgt, dt, tn, IR.R_CASE, T0=T, rc_want=-1))
            untouched(call(eng, entry, src, ds, tgt, dt, None, IR.R_CASE, T0=T, evaluate=True, rc_want=-1))
        untouched(call(eng, entry, src, ds, tgt, dt, None, IR.R_CASE, 1, rc_want=-1))                     # point-to-plane without normals
        for r in (0.0, -1.0, np.nan, np.inf, 1e-30, 1e30):
            untouched(call(eng, entry, src, ds, tgt, dt, tn, r, rc_want=-1))
        for est in (-1, 2):
            untouched(call(eng, entry, src, ds, tgt, dt, tn, IR.R_CASE, est, rc_want=-1))
        for maxit in (-1, 1001):
            untouched(call(eng, entry, src, ds, tgt, dt, tn, IR.R_CASE, 1, maxit, outs=("T", "stats", "corr"), rc_want=-1))
        untouched(call(eng, entry, src, ds, tgt, dt, tn, IR.R_CASE, rf=-1.0, rc_want=-1))
        untouched(call(eng, entry, src, ds, tgt, dt, tn, IR.R_CASE, rr=np.nan, rc_want=-1))
        untouched(call(eng, entry, src, ds, tgt, dt, tn, IR.R_CASE, origin=(0, np.nan, 0), rc_want=-1))
        assert b"sgm_register_icp" in _lib.load().sgm_last_error()
        same(call(eng, entry, src, ds, tgt, dt, tn, IR.R_CASE, 1, IR.SHAPE_ITERATIONS), IR.case_want(i, True, 1), entry)
    L = _lib.load()
    T = EYE.reshape(16).copy()
    st = np.full(8, MARK_S, np.uint64)
    o = np.zeros(3, F32)
    big = (1 << 24)
    assert L.sgm_register_icp(eng._h, src.ctypes.data, None, big, tgt.ctypes.data, None, None, 4, 0.1, o.ctypes.data, T.ctypes.data, 0, 1, 0.0, 0.0,
                              None, None, None, None, None, None, st.ctypes.data) == -4 and (st == MARK_S).all()      # SGM_ERR_UNSUPPORTED
    assert L.sgm_register_icp(eng._h, src.ctypes.data, None, -1, tgt.ctypes.data, None, None, 4, 0.1, o.ctypes.data, T.ctypes.data, 0, 1, 0.0, 0.0,
                              None, None, None, None, None, None, st.ctypes.data) == -1 and (st == MARK_S).all()


# ---- 5. sgm_transform_points and the Python surface ------------------------------------------------------------------------------------------
def test_transform_points_against_the_reference_in_place_included(eng):
    import torch
    rng = np.random.default_rng(12)
    T = IR.rigid((1, -2, 0.5), 33.0, (0.3, -4.0, 2.5))
    M = IR.m_of(T)
    for n in (1, 63, 257, 5000):
        xyz = (rng.standard_normal((n, 3)) * 3).astype(F32)
        nrm = rng.standard_normal((n, 3)).astype(F32)
        if n > 1:
            xyz[n // 2] = (np.nan, np.inf, 1.0)
        wx, wn = IR.transform(M, xyz), IR.transform_normals(M, nrm)
        gx, gn = eng.transform_points_host(xyz, T, nrm)
        assert np.array_equal(u32(gx), u32(wx)) and np.array_equal(u32(gn), u32(wn))
        gx, none = eng.transform_points_host(xyz, T)
        assert none is None and np.array_equal(u32(gx), u32(wx))
        tx, tn = torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda()
        ox = torch.zeros_like(tx)
        torch.cuda.synchronize()
        eng.transform_points_device(tx.data_ptr(), None, n, T, ox.data_ptr())
        eng.transform_points_device(tx.data_ptr(), tn.data_ptr(), n, T, tx.data_ptr(), tn.data_ptr())      # in place
        eng.synchronize()
        assert np.array_equal(u32(ox.cpu().numpy()), u32(wx)) and np.array_equal(u32(tx.cpu().numpy()), u32(wx))
        assert np.array_equal(u32(tn.cpu().numpy()), u32(wn))
    L = _lib.load()
    keep = np.full((4, 3), 7, F32)
    bad = EYE.reshape(16).copy()
    bad[15] = 2.0
    src = np.zeros((4, 3), F32)
    assert L.sgm_transform_points(eng._h, src.ctypes.data, None, 4, bad.ctypes.data, keep.ctypes.data, None) == -1 and (keep == 7).all()
    assert L.sgm_transform_points(eng._h, src.ctypes.data, src.ctypes.data, 4, EYE.reshape(16).ctypes.data, keep.ctypes.data, None) == -1
    assert (keep == 7).all() and b"sgm_transform_points" in L.sgm_last_error()


def test_the_python_surface_on_arrays_and_on_tensors():
    import torch
    src, tgt, tn, truth = IR.recovery_case()
    stats_of = lambda w: dict(zip(IR.STATS, [int(x) for x in w["stats"][:7]] + [sgm.pointcloud.ICP_STATUS[int(w["stats"][7])]]))
    w = ref(("recovery", 30, 1), src, None, tgt, None, tn, IR.R_CASE, estimation=1, max_iteration=30)
    T, fit, rmse = sgm.registration_icp(src, tgt, IR.R_CASE, target_normals=tn)
    assert T.shape == (4, 4) and T.dtype == np.float64 and u64(T).tolist() == u64(w["T"]).tolist() and (fit, rmse) == (w["fitness"], w["rmse"])
    T, fit, rmse, corr, d2, hist, st = sgm.registration_icp(src, tgt, IR.R_CASE, target_normals=tn, return_correspondences=True,
                                                            return_history=True, return_stats=True)
    assert np.array_equal(corr, w["corr"]) and np.array_equal(u32(d2), u32(w["d2"])) and u64(hist).tolist() == u64(w["history"]).tolist()
    assert st == stats_of(w) and st["status"] == "converged"
    w0 = ref(("recovery", 5, 0), src, None, tgt, None, tn, IR.R_CASE, estimation=0, max_iteration=5)
    T0, fit0, rmse0, st0 = sgm.registration_icp(src, tgt, IR.R_CASE, estimation="point_to_point", max_iteration=5, return_stats=True)
    assert u64(T0).tolist() == u64(w0["T"]).tolist() and st0 == stats_of(w0)
    # evaluate_registration under the result, and the merge
    we = IR.evaluate(IR.Clouds(src, None, tgt, None, None, IR.R_CASE), T, 0)
    f, r_, c, d = sgm.evaluate_registration(src, tgt, IR.R_CASE, T, return_correspondences=True)
    assert (f, r_) == (we["fitness"], we["rmse"]) == (fit, rmse) and np.array_equal(c, we["corr"]) and np.array_equal(u32(d), u32(we["d2"]))
    moved, mn = sgm.transform_points(src, T, normals=tn)
    assert np.array_equal(u32(moved), u32(IR.transform(IR.m_of(T), src))) and np.array_equal(u32(mn), u32(IR.transform_normals(IR.m_of(T), tn)))
    assert np.abs(moved - tgt).max() < 2e-6      # (a few binary32 ulp at coordinates up to 3.5)
    # XYZ images with their disparity maps
    i = IR.SHAPE_CASES.index((1000, 5000))
    s, ds, t, dt, n = IR.case_input(i)
    wi = IR.register(s, ds, t, dt, n, IR.R_CASE, estimation=1, max_iteration=3)
    Ti, fi, ri, ci, di = sgm.registration_icp(np.array(s).reshape(25, 40, 3), np.array(t).reshape(50, 100, 3), IR.R_CASE,
                                              target_normals=np.array(n).reshape(50, 100, 3), source_disparity=np.array(ds).reshape(25, 40),
                                              target_disparity=np.array(dt).reshape(50, 100), max_iteration=3, return_correspondences=True)
    assert u64(Ti).tolist() == u64(wi["T"]).tolist() and ci.shape == (25, 40) and np.array_equal(ci.reshape(-1), wi["corr"])
    assert np.array_equal(u32(di.reshape(-1)), u32(wi["d2"]))
    # HIP tensors stay on the device
    ts, tt, tnn = (torch.from_numpy(np.array(a)).cuda() for a in (src, tgt, tn))
    T2, fit2, rmse2, tc, td, st2 = sgm.registration_icp(ts, tt, IR.R_CASE, target_normals=tnn, return_correspondences=True, return_stats=True)
    assert tc.is_cuda and td.is_cuda and tc.dtype == torch.int32 and u64(T2).tolist() == u64(w["T"]).tolist() and st2 == stats_of(w)
    assert np.array_equal(tc.cpu().numpy(), w["corr"]) and np.array_equal(u32(td.cpu().numpy()), u32(w["d2"]))
    f2, r2 = sgm.evaluate_registration(ts, tt, IR.R_CASE, torch.from_numpy(T2))
    assert (f2, r2) == (fit, rmse)
    tm = sgm.transform_points(ts, T2)
    assert tm.is_cuda and np.array_equal(u32(tm.cpu().numpy()), u32(moved))
    with pytest.raises(sgm.error, match="both be numpy arrays or both be tensors"):
        sgm.registration_icp(ts, tgt, IR.R_CASE, target_normals=tn)
    with pytest.raises(sgm.error, match="float32 tensor of the target's shape"):
        sgm.registration_icp(ts, tt, IR.R_CASE, target_normals=tn)


def test_two_270_x_480_frames_from_the_pipeline_end_to_end():
    """two synthetic pairs of one scene geometry -- the second with another texture and other sensor noise, so its matching errors,
    its validity mask and its sub-pixel disparities are its own -- EACH through sgm_pipeline_device; the second cloud is then
    expressed in the frame of a rig moved by a known motion (a pair rendered from a moved viewpoint is not something synth.py can
    make).  Then voxel_down_sample -> estimate_normals_radius -> registration_icp -> transform_points against the reference: two
    independently reconstructed clouds, whose partners are not the points' own indices"""
    import torch
    H, W, D = 270, 480, 64
    e = Engine(U.params(D, 5, 0, 1))
    frames = []
    for seed in (5, 6):
        a, b = synth.make_pair(H, W, D, seed=seed)[:2]
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        dd = torch.empty((H, W), dtype=torch.int16, device="cuda")
        df = torch.empty((H, W), dtype=torch.float32, device="cuda")
        dx = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, synth.default_Q(W), dd.data_ptr(), df.data_ptr(), dx.data_ptr())
        e.synchronize()
        frames.append((dx.cpu().numpy(), df.cpu().numpy()))
    (xyz, disp), (xyz_b, disp_b) = frames
    assert not np.array_equal(disp, disp_b) and not np.array_equal(disp > 0, disp_b > 0)      # two reconstructions, not one
    ok = np.isfinite(xyz).all(axis=2) & (disp > 0)
    scale = float(np.median(np.abs(xyz[..., 2][ok])))
    voxel = float(F32(0.02 * scale))
    rig = IR.rigid((0.2, 1.0, 0.1), 0.7, (0.6 * voxel, -0.3 * voxel, 0.4 * voxel))
    xyz2 = sgm.transform_points(xyz_b, rig)                    # the second reconstruction in the moved rig's frame
    s, _ = sgm.voxel_down_sample(xyz, None, disp, voxel)
    t, _ = sgm.voxel_down_sample(xyz2, None, disp_b, voxel)
    n = sgm.estimate_normals_radius(t, None, 2 * voxel)
    assert s.shape[0] > 500 and t.shape[0] > 500
    w = IR.register(s, None, t, None, n, 2 * voxel, estimation=1, max_iteration=10)
    T, fit, rmse, corr, d2, st = sgm.registration_icp(s, t, 2 * voxel, target_normals=n, max_iteration=10, return_correspondences=True,
                                                       return_stats=True)
    assert u64(T).tolist() == u64(w["T"]).tolist() and (fit, rmse) == (w["fitness"], w["rmse"]) and st["iterations"] == int(w["stats"][3])
    assert np.array_equal(corr, w["corr"]) and np.array_equal(u32(d2), u32(w["d2"])) and st["correspondences"] == int(w["stats"][4])
    print("end to end: fitness", fit, "rmse / voxel", rmse / voxel, "iterations", st["iterations"], "status", st["status"],
          "points", s.shape[0], t.shape[0],
          "translation off the rig's / voxel", float(np.linalg.norm(T[:3, 3] - rig[:3, 3])) / voxel)
    assert fit > 0.5 and (corr[corr >= 0] != np.nonzero(corr >= 0)[0]).mean() > 0.5
    # the motion found is the rig's to within half of the voxel both clouds were thinned to (with the CPU oracle's maps in place of
    # the pipeline's, the same chain gives fitness 0.970, an rmse of 0.49 voxels, 6 iterations and 0.08 voxels here)
    assert np.linalg.norm(T[:3, 3] - rig[:3, 3]) < 0.5 * voxel
    merged = np.concatenate([sgm.transform_points(s, T), t])
    assert merged.shape == (s.shape[0] + t.shape[0], 3) and np.array_equal(u32(merged[:s.shape[0]]), u32(IR.transform(IR.m_of(T), s)))


# ---- 6. guarded buffers -------------------------------------------------------------------------------------------------------------------
def test_the_cases_with_every_buffer_guarded():
    """(the same cases ran in the plain mode above)"""
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "icp_guard_child.py")], capture_output=True, text=True, env=env,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"ICP_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) >= 8, tail
