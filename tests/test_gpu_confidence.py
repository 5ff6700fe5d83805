"""The per-pixel match confidence on the device (needs an MI355X): SGM_OPT_CONFIDENCE, the taps SGM_TAP_CONF_RAW and
SGM_TAP_CONF, sgm_bind_confidence_device and StereoSGBM.computeWithConfidence.

Yardstick: tests/confidence_ref.py on the aggregated volume S of the oracles (gray pairs in modes 0 and 1 -- the frozen
oracle; MODE_HH4 and colour pairs -- the volume oracle).  Every comparison is exact.  With the option on the
winner-take-all always runs as its own pass (k_wta_conf_t); which stages a row enqueues is read from the
profiled compute, not assumed."""
import os
import re
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

import bruteforce_color as BC
import confidence_ref as CR
import parity_util as U
from oracle import oracle as O
from oracle import volume_oracle as V
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd import stereo as cv
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U_LIST = (0, 1, 5, 10, 15, 25, 40, 70, 99, 100)

Row = namedtuple("Row", "H W D minD bs mode uniq sched debug cn")
R = Row
TAIL = " select_lr median3 speckle*4 conf _wall*0"
# rows; `route`: the stages in front of the epilogue where the row pins them (shapes of tests/test_gpu_paths.py's table)
ROWS = [
    (R(40, 300, 16, 0, 5, 0, 10, 1, 0, 1), "features cost_pix cost_box paths5 wta_conf"),                       # 5 volumes
    (R(40, 300, 32, 0, 5, 0, 10, 1, 8192, 1), "features cost_pix cost_box path_W path_E prepass_dn sweep_dn wta_conf"),  # 3 volumes
    (R(41, 301, 48, -3, 5, 0, 0, 1, 0, 1), None),                                                               # 5 volumes, idle lanes in a group
    (R(40, 300, 64, 0, 5, 1, 10, 1, 0, 1), None),                                                               # MODE_HH, small-D schedule
    (R(38, 333, 96, 2, 3, 0, 100, 1, 0, 1), None),                                                              # 2 volumes, any-D staging, weight 0
    (R(40, 300, 128, 0, 5, 0, 150, 1, 0, 1), "features cost_pix cost_box path_W prepass_dn sweep_dn wta_conf"),  # 2 volumes, negative weight
    (R(40, 300, 128, 0, 5, 0, 10, 1, 65536, 1), "features cost_pix cost_box prepass_dn sweep_dn path_W wta_conf"),
    (R(40, 300, 256, 0, 5, 0, 10, 1, 0, 1), "features cost_pix cost_box prepass_dn sweep_dn path_W wta_conf"),   # fuses by default: diverted
    (R(40, 300, 256, 0, 5, 0, 10, 1, 2048, 1), "features cost_pix cost_box prepass_dn sweep_dn path_W wta_conf"),
    (R(29, 640, 160, 5, 5, 0, 10, 1, 0, 1), None),                                                              # diverted, any-D staging
    (R(40, 300, 256, 0, 5, 1, 10, 1, 0, 1), "features cost_pix cost_box prepass_dn prepass_up sweep_dn sweep_up wta_conf"),
    (R(45, 420, 256, -7, 7, 1, 100, 1, 0, 1), None),
    (R(40, 300, 128, 0, 5, 1, 10, 1, 2, 1), "features cost_pix cost_box prepass_dn prepass_up sweep_dn sweep_up wta_conf"),  # debug 2 asks for the fused form: diverted
    (R(33, 700, 512, 0, 3, 1, 0, 1, 0, 1), None),
    (R(9, 783, 528, 0, 5, 1, 10, 1, 0, 1), None),                                                               # D > 512: one kernel per direction
    (R(9, 1153, 1024, 0, 5, 0, 100, 2, 0, 1), None),
    (R(40, 300, 64, 0, 5, 0, 10, 0, 0, 1), "features cost_pix cost_box path_S path_SE path_SW path_E path_W wta_conf"),
    (R(40, 300, 64, 0, 5, 1, 150, 0, 0, 1),
     "features cost_pix cost_box path_S path_SE path_SW path_N path_NE path_NW path_E path_W wta_conf"),
    (R(40, 300, 256, 0, 5, 1, 10, 2, 0, 1), "features cost_pix cost_box chain_dn chain_up wta_conf"),
    (R(40, 300, 128, 0, 5, 0, 10, 2, 0, 1), "features cost_pix cost_box path_W chain_dn wta_conf"),
    (R(40, 300, 32, 0, 5, 0, 10, 2, 0, 1), "features cost_pix cost_box paths5 wta_conf"),
    (R(40, 300, 32, 0, 5, 0, 10, 1, 4, 1), "features cost_hsum cost_vsum prepass_dn sweep_dn path_W wta_conf"),  # no lane groups
    (R(40, 300, 64, 0, 5, 1, 10, 1, 8 | 256, 1), None),
    (R(40, 300, 16, 0, 5, 1, 10, 1, 16, 1), None),
    (R(40, 300, 32, 0, 5, 0, 10, 1, 4096, 1), None),
    (R(40, 300, 48, -3, 5, 3, 10, 1, 0, 1), None),                                                              # MODE_HH4: 4 volumes
    (R(40, 300, 192, 0, 5, 3, 10, 1, 0, 1), None),
    (R(40, 300, 128, 4, 3, 3, 100, 0, 0, 1), None),
    (R(40, 300, 128, 0, 5, 3, 10, 2, 0, 1), None),
    (R(30, 260, 32, 0, 3, 0, 10, 1, 0, 3), None),                                                               # colour
    (R(32, 420, 192, -5, 5, 1, 15, 1, 0, 3), None),
    (R(30, 300, 64, 0, 5, 3, 10, 2, 0, 3), None),
    (R(20, 60, 64, 0, 5, 0, 10, 1, 0, 1), "fill_invalid"),                                                      # no column can be matched
]
row_id = lambda r: f"{r.H}x{r.W} D{r.D} minD{r.minD} mode{r.mode} u{r.uniq} sched{r.sched} dbg{r.debug}{' colour' if r.cn == 3 else ''}"


def _pair(r, seed):
    if r.cn == 3:
        return BC.colour_pair(r.H, r.W, r.D, seed=seed, minD=r.minD)
    return synth.make_pair(r.H, r.W, r.D, seed)[:2]


def _params(r, **kw):
    p = U.params(r.D, r.bs, r.minD, r.mode, penalty="plain" if r.cn == 3 else "notebook", uniquenessRatio=r.uniq,
                 speckleWindowSize=30, speckleRange=2)
    p.update(kw)
    return p


def _oracle(r, a, b, p):
    return (V if r.cn == 3 or r.mode == 3 else O).sgbm_compute(a, b, taps=True, **p)


def _reference(r, t, disp):
    """(conf_raw, conf) of a row from the oracle's taps and final map"""
    if "S" not in t:
        z = np.zeros((r.H, r.W), np.uint8)
        return z, z
    minX1 = r.W - t["S"].shape[1] + min(r.minD, 0)
    raw = CR.conf_raw(t["S"], r.W, minX1)
    return raw, CR.conf_final(raw, disp, r.minD)


def _engine(r, p, conf):
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, r.sched)
    if r.debug:
        eng.set_option(_lib.SGM_OPT_DEBUG, r.debug)
    eng.set_option(_lib.SGM_OPT_CONFIDENCE, int(conf))
    return eng


def _run(r, a, b, p, conf):
    eng = _engine(r, p, conf)
    eng.set_option(_lib.SGM_OPT_PROFILE, 1)
    out = dict(disp=eng.compute_host(a, b))
    out["disp_raw"] = eng.tap(_lib.SGM_TAP_DISP_RAW, r.H, r.W)
    out["disp_median"] = eng.tap(_lib.SGM_TAP_DISP_MEDIAN, r.H, r.W)
    out["headroom"] = eng.headroom()
    out["stages"] = " ".join(n if k == 1 else f"{n}*{k}" for n, _, k in eng.stage_times())
    if conf:
        out["conf_raw"] = eng.tap(_lib.SGM_TAP_CONF_RAW, r.H, r.W)
        out["conf"] = eng.tap(_lib.SGM_TAP_CONF, r.H, r.W)
    return out, eng


@pytest.mark.parametrize("r,route", ROWS, ids=[row_id(r) for r, _ in ROWS])
def test_taps_match_the_reference_and_the_disparity_outputs_do_not_move(r, route):
    a, b = _pair(r, 8100 + r.D + r.mode)
    p = _params(r)
    want, t = _oracle(r, a, b, p)
    assert t["headroom_ok"]
    raw, conf = _reference(r, t, want)
    on, _ = _run(r, a, b, p, True)
    off, eng_off = _run(r, a, b, p, False)
    # both taps
    assert on["conf_raw"].dtype == np.uint8 and on["conf_raw"].shape == (r.H, r.W)
    assert np.array_equal(on["conf_raw"], raw), U.describe_mismatch("conf_raw", on["conf_raw"], raw)
    assert np.array_equal(on["conf"], conf), U.describe_mismatch("conf", on["conf"], conf)
    if "S" in t:
        assert CR.deciles_populated(raw) >= 5 and (conf != raw).any()       # not a degenerate row
    # the disparity outputs and the headroom record: the oracle's, and the same bits with the option off
    assert np.array_equal(on["disp"], want)
    for k in ("disp", "disp_raw", "disp_median"):
        assert np.array_equal(on[k], off[k]), k
    assert on["headroom"] == off["headroom"] == dict(ok=True, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"])
    # the route: one winner-take-all of its own with the byte, none fused into a path kernel, the epilogue last
    names = [s.split("*")[0] for s in on["stages"].split()]
    assert "conf" in names and not [n for n in names if n.endswith("_wta")], on["stages"]
    if "S" in t:
        assert names.count("wta_conf") == 1 and "wta" not in names, on["stages"]
        assert names[names.index("wta_conf") - 1] in ("paths5", "paths4", "sweep_dn", "sweep_up", "chain_dn", "chain_up", "path_W"), on["stages"]
    if route is not None:
        tail = TAIL if "S" in t else " median3 speckle*4 conf _wall*0"
        assert on["stages"] == route + tail
    # option off: no stage of the option, and the taps are refused
    assert "conf" not in off["stages"].split() and "wta_conf" not in off["stages"]
    for tap in (_lib.SGM_TAP_CONF_RAW, _lib.SGM_TAP_CONF):
        with pytest.raises(cv.error, match="SGM_OPT_CONFIDENCE"):
            eng_off.tap(tap, r.H, r.W)


def test_every_route_with_a_winner_take_all_of_its_own_is_in_the_table():
    """k_wta_conf_t over 1, 2, 3, 4 and 5 volumes, behind the small-D kernels, the fused and the chained sweeps, the in-row
    path on the main stream, and the one-kernel-per-direction schedule (also as D > 512 takes it); both signs of the weight."""
    plans = []
    for r, _ in ROWS:
        if r.W + min(r.minD, 0) - max(r.minD + r.D, 0) <= 0:
            continue
        q = _lib.debug_plan(_params(r), r.H, r.W, r.cn, r.sched, debug=r.debug | 2048)     # 2048: the separate pass, as the option forces it
        plans.append((r, q))
    # (schedule 0 and D > 512 fuse whatever debug says: the option alone diverts them -- those rows are pinned by their stages)
    for nv in (1, 2, 3, 4, 5):
        assert any(q["nvol"] == nv and not q["fused_wta"] for _, q in plans), nv
    assert any(q["chain"] for _, q in plans) and any(q["rows4"] for _, q in plans)
    assert any(r.sched == 0 for r, _ in plans) and any(r.D > 512 for r, _ in plans)
    assert {True, False} == {r.uniq < 100 for r, _ in plans}
    assert {10} < {r.uniq for r, _ in plans} >= {0, 100, 150}
    assert {r.D for r, _ in plans} >= {16, 32, 48, 64, 96, 128, 256, 512, 528, 1024}


@pytest.mark.parametrize("H,W,D,minD,mode,bs,sched,seed", [(40, 200, 64, 0, 0, 5, 1, 11), (33, 150, 32, -3, 1, 5, 1, 12),
                                                           (30, 180, 128, 0, 1, 3, 2, 13), (40, 420, 256, 0, 0, 5, 1, 14)])
def test_conf_raw_is_the_largest_ratio_that_keeps_the_pixel_on_the_device(H, W, D, minD, mode, bs, sched, seed):
    """engines that differ only in uniquenessRatio (LR check off: disp12MaxDiff = 100000) return the same conf_raw, and
    disp_raw is valid exactly where conf_raw >= u"""
    a, b, _ = synth.make_pair(H, W, D, seed)
    first = None
    for u in U_LIST:
        r = R(H, W, D, minD, bs, mode, u, sched, 0, 1)
        p = _params(r, disp12MaxDiff=100000, speckleWindowSize=0, speckleRange=0)
        out, eng = _run(r, a, b, p, True)
        minX1, W1 = eng.geometry(W)
        if first is None:
            first = out["conf_raw"]
            _, t = O.sgbm_compute(a, b, taps=True, **p)
            assert t["headroom_ok"] and (t["S"].min(axis=2) != CR.MAX_COST).all()
            assert CR.deciles_populated(first[:, minX1:minX1 + W1]) >= 8
        assert np.array_equal(out["conf_raw"], first), u
        valid = out["disp_raw"] != (minD - 1) * 16
        cols = np.zeros((H, W), bool)
        cols[:, minX1:minX1 + W1] = True
        assert np.array_equal(valid, (first >= u) & cols), (u, int((valid != ((first >= u) & cols)).sum()))


# ---- the device binding ------------------------------------------------------------------------------------------------------
def _resident(pairs, H, W):
    import torch
    dev = torch.device("cuda", 0)
    dl = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a, _ in pairs]
    dr = [torch.from_numpy(np.ascontiguousarray(b)).to(dev) for _, b in pairs]
    dd = [torch.full((H, W), -7, dtype=torch.int16, device=dev) for _ in pairs]
    dc = [torch.full((H, W), 0xEE, dtype=torch.uint8, device=dev) for _ in pairs]
    torch.cuda.synchronize()
    return dl, dr, dd, dc


ptr = lambda ts: [t.data_ptr() for t in ts]


def _single(p, a, b, H, W, sched=1):
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, sched)
    eng.set_option(_lib.SGM_OPT_CONFIDENCE, 1)
    d = eng.compute_host(a, b)
    return d, eng.tap(_lib.SGM_TAP_CONF, H, W)


def test_binding_of_the_single_pair_entries_is_consumed_by_one_call():
    H, W, D = 40, 300, 128
    p = U.params(D, 5, 0, 1, speckleWindowSize=30, speckleRange=2)
    pairs = [synth.make_pair(H, W, D, 8300)[:2]]
    want_d, want_c = _single(p, *pairs[0], H, W)
    assert np.array_equal(want_d, O.sgbm_compute(*pairs[0], **p)) and (want_c > 0).any()
    dl, dr, dd, dc = _resident(pairs, H, W)
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_CONFIDENCE, 1)
    for entry in ("compute", "pipeline"):
        dc[0].fill_(0xEE)
        if entry == "compute":
            eng.compute_device(dl[0].data_ptr(), dr[0].data_ptr(), H, W, W, dd[0].data_ptr(), d_conf=dc[0].data_ptr())
        else:
            eng.pipeline_device(dl[0].data_ptr(), dr[0].data_ptr(), H, W, W, None, dd[0].data_ptr(), None, None, d_conf=dc[0].data_ptr())
        eng.synchronize()
        assert np.array_equal(dd[0].cpu().numpy(), want_d) and np.array_equal(dc[0].cpu().numpy(), want_c), entry
        # the map went to the bound pointer: the engine's own buffer does not hold it, conf_raw is there
        with pytest.raises(cv.error, match="bound"):
            eng.tap(_lib.SGM_TAP_CONF, H, W)
        assert (eng.tap(_lib.SGM_TAP_CONF_RAW, H, W) >= want_c).all()
        # consumed: the next call without a new binding writes nothing there, and its map is in the engine again
        dc[0].fill_(0x5A)
        eng.compute_device(dl[0].data_ptr(), dr[0].data_ptr(), H, W, W, dd[0].data_ptr())
        eng.synchronize()
        assert (dc[0].cpu().numpy() == 0x5A).all(), entry
        assert np.array_equal(eng.tap(_lib.SGM_TAP_CONF, H, W), want_c)


@pytest.mark.parametrize("sched,gmax", [(1, 0), (2, 0), (2, 2), (2, 3)])
def test_binding_of_the_batch_entry(sched, gmax):
    """5 pairs: pair after pair (schedule 1), one chained group, groups of 2 + 2 + 1 and of 3 + 2 -- each pair's map equals
    the single-pair result for that pair; a second call without a binding leaves the sentinel alone"""
    H, W, D, N = 40, 300, 128, 5
    p = U.params(D, 5, 0, 1, speckleWindowSize=30, speckleRange=2)
    pairs = [synth.make_pair(H, W, D, 8400 + i)[:2] for i in range(N)]
    singles = [_single(p, a, b, H, W, sched) for a, b in pairs]
    dl, dr, dd, dc = _resident(pairs, H, W)
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, sched)
    eng.set_option(_lib.SGM_OPT_SWEEP_ROWS, 4)
    eng.set_option(_lib.SGM_OPT_GROUP_MAX, gmax)
    eng.set_option(_lib.SGM_OPT_CONFIDENCE, 1)
    eng.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, None, ptr(dd), d_confs=ptr(dc))
    eng.synchronize()
    for i in range(N):
        assert np.array_equal(dd[i].cpu().numpy(), singles[i][0]), i
        assert np.array_equal(dc[i].cpu().numpy(), singles[i][1]), (i, int((dc[i].cpu().numpy() != singles[i][1]).sum()))
    assert len({s[1].tobytes() for s in singles}) == N                     # five different maps
    for c in dc:
        c.fill_(0x5A)
    eng.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, None, ptr(dd))
    eng.synchronize()
    assert all((c.cpu().numpy() == 0x5A).all() for c in dc)
    assert all(np.array_equal(dd[i].cpu().numpy(), singles[i][0]) for i in range(N))


def test_binding_error_returns():
    H, W, D = 40, 300, 64
    p = U.params(D, 5, 0, 0, speckleWindowSize=30, speckleRange=2)
    pairs = [synth.make_pair(H, W, D, 8500 + i)[:2] for i in range(3)]
    dl, dr, dd, dc = _resident(pairs, H, W)
    eng = Engine(p)
    with pytest.raises(cv.error, match="SGM_OPT_CONFIDENCE"):               # option off
        eng.bind_confidence_device(ptr(dc[:1]))
    with pytest.raises(cv.error, match="SGM_OPT_CONFIDENCE 2"):             # values other than 0 and 1
        eng.set_option(_lib.SGM_OPT_CONFIDENCE, 2)
    with pytest.raises(cv.error):
        eng.set_option(_lib.SGM_OPT_CONFIDENCE, -1)
    eng.set_option(_lib.SGM_OPT_CONFIDENCE, 1)
    with pytest.raises(cv.error, match="pair 1"):                           # a null pointer
        eng.bind_confidence_device([dc[0].data_ptr(), 0, dc[2].data_ptr()])
    # N differs from the call's pair count: reported by the image call, which consumes the binding all the same
    eng.bind_confidence_device(ptr(dc[:2]))
    with pytest.raises(cv.error, match="bound 2 maps"):
        eng.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, None, ptr(dd))
    eng.bind_confidence_device(ptr(dc))
    with pytest.raises(cv.error, match="bound 3 maps"):
        eng.compute_device(dl[0].data_ptr(), dr[0].data_ptr(), H, W, W, dd[0].data_ptr())
    # a failing image call consumes it too (stride smaller than a row), and N = 0 clears one
    eng.bind_confidence_device(ptr(dc[:1]))
    with pytest.raises(cv.error, match="stride"):
        eng.compute_device(dl[0].data_ptr(), dr[0].data_ptr(), H, W, W - 1, dd[0].data_ptr())
    eng.bind_confidence_device(ptr(dc[:1]))
    eng.bind_confidence_device([])
    for c in dc:
        c.fill_(0x5A)
    eng.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, None, ptr(dd))     # the engine is usable, nothing is bound
    eng.synchronize()
    assert all((c.cpu().numpy() == 0x5A).all() for c in dc)
    assert np.array_equal(dd[2].cpu().numpy(), O.sgbm_compute(*pairs[2], **p))
    # the host batch entry computes as before with the option on (no per-pair confidence from it)
    disps = eng.compute_batch_host(np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]))
    assert all(np.array_equal(disps[i], O.sgbm_compute(*pairs[i], **p)) for i in range(3))


# ---- the Python surface ----------------------------------------------------------------------------------------------------
def test_compute_with_confidence_and_the_cached_engine():
    import torch
    H, W, D = 40, 300, 64
    p = U.params(D, 5, 0, 0, speckleWindowSize=30, speckleRange=2)
    a, b, _ = synth.make_pair(H, W, D, 8600)
    want, t = O.sgbm_compute(a, b, taps=True, **p)
    raw, conf = _reference(R(H, W, D, 0, 5, 0, 10, 1, 0, 1), t, want)
    m = cv.StereoSGBM_create(**p)
    d, c = m.computeWithConfidence(a, b)
    assert isinstance(c, np.ndarray) and c.dtype == np.uint8 and c.shape == (H, W)
    assert np.array_equal(d, want) and np.array_equal(c, conf)
    # the cached engine is back to not producing the map: plain compute() does not pay for it
    eng = cv.get_engine(p)
    eng.set_option(_lib.SGM_OPT_PROFILE, 1)
    assert np.array_equal(m.compute(a, b), want)
    names = [n for n, _, _ in eng.stage_times()]
    assert "conf" not in names and "wta_conf" not in names, names
    with pytest.raises(cv.error, match="SGM_OPT_CONFIDENCE"):
        eng.tap(_lib.SGM_TAP_CONF, H, W)
    eng.set_option(_lib.SGM_OPT_PROFILE, 0)
    # HIP tensors in, tensors out; a colour pair through the same validation
    dev = torch.device("cuda", 0)
    dt, ct = m.computeWithConfidence(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
    assert ct.dtype == torch.uint8 and ct.is_cuda and np.array_equal(dt.cpu().numpy(), want) and np.array_equal(ct.cpu().numpy(), conf)
    L3, R3 = BC.colour_pair(30, 260, 32, seed=8601)
    p3 = U.params(32, 3, 0, 1, penalty="plain", speckleWindowSize=30, speckleRange=2)
    w3, t3 = V.sgbm_compute(L3, R3, taps=True, **p3)
    d3, c3 = cv.StereoSGBM_create(**p3).computeWithConfidence(L3, R3)
    assert np.array_equal(d3, w3) and np.array_equal(c3, _reference(R(30, 260, 32, 0, 3, 1, 10, 1, 0, 3), t3, w3)[1])
    with pytest.raises(cv.error):
        m.computeWithConfidence(a, b[:, :-1])
    # the consumer: thinning the cloud after the fact equals numpy's boolean indexing with the extra condition
    import stereo_reconstruction_cv_amd as pkg
    f = eng.disp_to_float_host(d)
    xyz = pkg.reprojectImageTo3D(f, synth.default_Q(W))
    colors = np.stack([a, a, a], axis=-1)
    base = ~np.isnan(xyz[..., 0]) & ~np.isinf(xyz[..., 0]) & (f > 0)
    pts0, col0 = pkg.valid_points(xyz, colors, f)
    assert np.array_equal(pts0, xyz[base]) and np.array_equal(col0, colors[base])
    for u in (0, 30, 101):
        pts, col = pkg.valid_points(xyz, colors, f, confidence=c, min_confidence=u)
        mask = base & (c >= u)
        assert np.array_equal(pts, xyz[mask]) and np.array_equal(col, colors[mask]), u
    assert 0 < (base & (c >= 30)).sum() < base.sum()


# ---- history, guarded buffers ------------------------------------------------------------------------------------------------
def test_one_engine_alternating_option_and_shapes_then_from_poisoned_buffers():
    p = U.params(64, 5, 0, 1, speckleWindowSize=30, speckleRange=2)
    shapes = [(60, 420), (24, 200), (60, 420), (33, 310)]
    cases = []
    for i, (H, W) in enumerate(shapes):
        a, b, _ = synth.make_pair(H, W, 64, 8700 + i)
        want, t = O.sgbm_compute(a, b, taps=True, **p)
        cases.append((a, b, want) + _reference(R(H, W, 64, 0, 5, 1, 10, 1, 0, 1), t, want))
    eng = Engine(p)
    try:
        for rnd in range(2):
            if rnd == 1:
                eng.set_option(_lib.SGM_OPT_POISON, 0xA5)
            for i, (a, b, want, raw, conf) in enumerate(cases):
                for on in (1, 0, 1):
                    eng.set_option(_lib.SGM_OPT_CONFIDENCE, on)
                    assert np.array_equal(eng.compute_host(a, b), want), (rnd, i, on)
                    if on:
                        assert np.array_equal(eng.tap(_lib.SGM_TAP_CONF_RAW, *a.shape), raw), (rnd, i)
                        assert np.array_equal(eng.tap(_lib.SGM_TAP_CONF, *a.shape), conf), (rnd, i)
                    else:
                        with pytest.raises(cv.error, match="SGM_OPT_CONFIDENCE"):
                            eng.tap(_lib.SGM_TAP_CONF, *a.shape)
                    if rnd == 1:
                        eng.set_option(_lib.SGM_OPT_POISON, 0xA5)
    finally:
        eng.set_option(_lib.SGM_OPT_POISON, -1)


def test_confidence_rows_with_every_buffer_guarded():
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "confidence_guard_child.py")], capture_output=True, text=True,
                       env=env, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"CONF_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) == 7, tail


# ---- full size ---------------------------------------------------------------------------------------------------------------
def test_4k_d256_hh_final_map_against_the_oracle():
    H, W, D = 2160, 3840, 256
    p = U.params(D, 7, 0, 1)
    a, b, _ = synth.make_pair(H, W, D, 8800)
    ws = O.workspace(H, W, **p)
    want = O.sgbm_compute(a, b, workspace=ws, **p)
    minX1 = W - ws["S"].shape[1]
    raw = CR.conf_raw(ws["S"], W, minX1)
    del ws
    conf = CR.conf_final(raw, want, 0)
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_CONFIDENCE, 1)
    got = eng.compute_host(a, b)
    assert eng.headroom()["ok"]
    assert np.array_equal(got, want)
    c = eng.tap(_lib.SGM_TAP_CONF, H, W)
    assert np.array_equal(c, conf), U.describe_mismatch("conf", c, conf)
    assert np.array_equal(eng.tap(_lib.SGM_TAP_CONF_RAW, H, W), raw)
    assert CR.deciles_populated(conf) >= 8


def test_1080p_d128_sgbm_batch_of_four_through_the_binding():
    H, W, D, N = 1080, 1920, 128, 4
    p = U.params(D, 5, 0, 0)
    pairs = [synth.make_pair(H, W, D, 8900 + i)[:2] for i in range(N)]
    dl, dr, dd, dc = _resident(pairs, H, W)
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, 2)
    eng.set_option(_lib.SGM_OPT_CONFIDENCE, 1)
    eng.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, None, ptr(dd), d_confs=ptr(dc))
    eng.synchronize()
    assert eng.headroom()["ok"]
    for i, (a, b) in enumerate(pairs):
        want, t = O.sgbm_compute(a, b, taps=True, **p)
        assert t["headroom_ok"]
        _, conf = _reference(R(H, W, D, 0, 5, 0, 10, 2, 0, 1), t, want)
        del t
        assert np.array_equal(dd[i].cpu().numpy(), want), i
        got = dc[i].cpu().numpy()
        assert np.array_equal(got, conf), (i, U.describe_mismatch("conf", got, conf))
