"""The right-view disparity map on the device (needs an MI355X): SGM_OPT_RIGHT_VIEW, the taps SGM_TAP_RIGHT_RAW and
SGM_TAP_RIGHT, sgm_bind_right_device and StereoSGBM.computeLeftRight.

Yardstick: tests/right_view_ref.py on the aggregated volume S of the oracles (gray pairs in modes 0 and 1 -- the frozen
oracle; MODE_HH4 and colour pairs -- the volume oracle).  Every comparison is exact.  With the option on the left
winner-take-all always runs as its own pass, so that S is in device memory for the diagonal one (k_right_wta, DESIGN.md
4.13); the left outputs must be the bits of an option-off run."""
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
import right_view_ref as RR
from oracle import oracle as O
from oracle import volume_oracle as V
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd import stereo as cv
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Row = namedtuple("Row", "H W D minD bs mode uniq d12 speckle sched debug cn")
R = Row
# the parity rows: the smallest shapes at which the diagonal can go wrong
BASE = [
    R(40, 200, 64, 0, 5, 0, 10, 1, 1, 1, 0, 1),        # five volumes
    R(33, 150, 32, -3, 5, 1, 10, 1, 1, 1, 0, 1),
    R(21, 300, 128, 5, 5, 0, 10, 1, 1, 1, 0, 1),       # S + S2
    R(24, 90, 64, 0, 5, 1, 10, 1, 1, 1, 0, 1),         # W1 = 26 < D: every pixel truncated
    R(8, 17, 16, 0, 3, 0, 10, 1, 1, 1, 0, 1),          # W1 = 1
    R(8, 16, 16, 0, 3, 0, 10, 1, 1, 1, 0, 1),          # no matched column
    R(19, 700, 256, 0, 5, 1, 10, 1, 1, 1, 0, 1),
    R(17, 1100, 512, 0, 3, 3, 10, 1, 1, 1, 0, 1),
    R(9, 1300, 1024, 0, 3, 1, 10, 1, 1, 1, 0, 1),      # NP = 8
    R(13, 531, 48, 0, 5, 1, 10, 1, 1, 1, 0, 1),        # D not a power of two, ragged tile tail
    R(40, 200, 64, 0, 5, 0, 10, 1, 1, 1, 0, 3),        # colour pair
]
# further coverage over these rows: ratios, disp12MaxDiff, speckle off, schedules, the debug bits that select a fused-WTA route
MORE = [
    BASE[0]._replace(uniq=0, d12=-1), BASE[0]._replace(uniq=100, d12=0, speckle=0), BASE[0]._replace(uniq=150, d12=100000),
    BASE[0]._replace(sched=0), BASE[0]._replace(sched=2), BASE[0]._replace(debug=4),                   # v1; small D; no lane groups: fused
    BASE[1]._replace(uniq=100, sched=0), BASE[1]._replace(d12=100000, speckle=0, sched=2),
    BASE[2]._replace(uniq=0, sched=2), BASE[2]._replace(debug=2, mode=1), BASE[2]._replace(uniq=150, debug=65536),
    BASE[3]._replace(uniq=100, d12=100000), BASE[3]._replace(uniq=0, sched=0),
    BASE[6]._replace(mode=0), BASE[6]._replace(mode=0, uniq=150, sched=2), BASE[6]._replace(sched=2, d12=0), BASE[6]._replace(sched=0, uniq=0),
    BASE[7]._replace(mode=0, uniq=100), BASE[8]._replace(uniq=150, speckle=0), BASE[8]._replace(mode=0, sched=2, uniq=0),
    BASE[9]._replace(mode=3, d12=-1), BASE[9]._replace(mode=0, minD=-7, uniq=0), BASE[10]._replace(mode=1, sched=2, uniq=100),
    R(23, 260, 160, 2, 5, 0, 10, 1, 1, 1, 0, 1),       # MODE_SGBM, D > 128 and no power of two: fuses by default
    R(22, 210, 32, 0, 5, 0, 10, 1, 1, 1, 8192, 1),     # three volumes
]
ROWS = BASE + MORE
row_id = lambda r: (f"{r.H}x{r.W} D{r.D} minD{r.minD} mode{r.mode} u{r.uniq} d12_{r.d12} sp{r.speckle} sched{r.sched} dbg{r.debug}"
                    f"{' colour' if r.cn == 3 else ''}")


def _pair(r, seed):
    if r.cn == 3:
        return BC.colour_pair(r.H, r.W, r.D, seed=seed, minD=r.minD)
    return synth.make_pair(r.H, r.W, r.D, seed)[:2]


def _params(r, **kw):
    p = U.params(r.D, r.bs, r.minD, r.mode, penalty="plain" if r.cn == 3 else "notebook", uniquenessRatio=r.uniq,
                 disp12MaxDiff=r.d12, speckleWindowSize=30 if r.speckle else 0, speckleRange=2 if r.speckle else 0)
    p.update(kw)
    return p


def _oracle(r, a, b, p):
    return (V if r.cn == 3 or r.mode == 3 else O).sgbm_compute(a, b, taps=True, **p)


def _reference(r, t, p):
    """(right_raw, right) of a row from the oracle's taps"""
    if "S" not in t:
        z = RR.all_invalid(r.H, r.W, r.minD)
        return z, z
    minX1 = r.W - t["S"].shape[1] + min(r.minD, 0)
    return RR.right_view(t["S"], r.W, minX1, p)


def _engine(r, p, on, conf=0):
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, r.sched)
    if r.debug:
        eng.set_option(_lib.SGM_OPT_DEBUG, r.debug)
    eng.set_option(_lib.SGM_OPT_RIGHT_VIEW, int(on))
    eng.set_option(_lib.SGM_OPT_CONFIDENCE, int(conf))
    return eng


def _run(r, a, b, p, on, conf=0):
    eng = _engine(r, p, on, conf)
    eng.set_option(_lib.SGM_OPT_PROFILE, 1)
    out = dict(disp=eng.compute_host(a, b))
    out["disp_raw"] = eng.tap(_lib.SGM_TAP_DISP_RAW, r.H, r.W)
    out["disp_median"] = eng.tap(_lib.SGM_TAP_DISP_MEDIAN, r.H, r.W)
    out["headroom"] = eng.headroom()
    out["stages"] = [n for n, _, _ in eng.stage_times()]
    if on:
        out["right_raw"] = eng.tap(_lib.SGM_TAP_RIGHT_RAW, r.H, r.W)
        out["right"] = eng.tap(_lib.SGM_TAP_RIGHT, r.H, r.W)
    return out, eng


@pytest.mark.parametrize("r", ROWS, ids=[row_id(r) for r in ROWS])
def test_taps_match_the_reference_and_the_left_outputs_do_not_move(r):
    a, b = _pair(r, 9100 + r.D + r.mode)
    p = _params(r)
    want, t = _oracle(r, a, b, p)
    assert t["headroom_ok"]
    raw, fin = _reference(r, t, p)
    on, _ = _run(r, a, b, p, True)
    off, eng_off = _run(r, a, b, p, False)
    assert on["right_raw"].dtype == np.int16 and on["right_raw"].shape == (r.H, r.W)
    assert np.array_equal(on["right_raw"], raw), U.describe_mismatch("right_raw", on["right_raw"], raw)
    assert np.array_equal(on["right"], fin), U.describe_mismatch("right", on["right"], fin)
    INV = (r.minD - 1) * 16
    if "S" in t and t["S"].shape[1] > 1:
        assert (raw != INV).any() and (raw == INV).any()                      # not a degenerate row
    # the left outputs and the headroom record: the oracle's, and the same bits with the option off
    assert np.array_equal(on["disp"], want)
    for k in ("disp", "disp_raw", "disp_median"):
        assert np.array_equal(on[k], off[k]), k
    assert on["headroom"] == off["headroom"] == dict(ok=True, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"])
    # the stages: named, behind the left epilogue, no winner-take-all fused into a path kernel; none with the option off
    tail = (["right_wta", "right_check"] if "S" in t else ["right_fill_invalid"]) + ["right_median3"] + (["right_speckle"] if r.speckle else [])
    assert on["stages"][-len(tail) - 1:-1] == tail and on["stages"][-1] == "_wall", on["stages"]
    assert on["stages"][-len(tail) - 2] == ("speckle" if r.speckle else "median3"), on["stages"]
    assert not [n for n in on["stages"] if n.endswith("_wta") and n != "right_wta"], on["stages"]
    assert not [n for n in off["stages"] if n.startswith("right_")], off["stages"]
    for tap in (_lib.SGM_TAP_RIGHT_RAW, _lib.SGM_TAP_RIGHT):
        with pytest.raises(cv.error, match="SGM_OPT_RIGHT_VIEW"):
            eng_off.tap(tap, r.H, r.W)


def test_every_route_that_fuses_the_winner_take_all_by_default_is_in_the_table():
    """schedule 0, MODE_SGBM with D > 128 (power of two and not), D > 512, and the debug bits that ask for the fused form
    (2; 4 in MODE_SGBM) -- each is diverted by the option; and the separate routes over 1 .. 5 volumes, chained
    and not, are there too, with both signs of the uniqueness weight and every disp12MaxDiff class"""
    fused, sep = [], []
    for r in ROWS:
        if r.W + min(r.minD, 0) - max(r.minD + r.D, 0) <= 0:
            continue
        q = _lib.debug_plan(_params(r), r.H, r.W, r.cn, r.sched, debug=r.debug)
        qo = _lib.debug_plan(_params(r), r.H, r.W, r.cn, r.sched, debug=r.debug, right_view=1)
        assert qo["fused_wta"] == 0, r
        (fused if q["fused_wta"] else sep).append((r, q, qo))
    assert any(r.sched == 0 and r.D <= 512 for r, _, _ in fused)
    assert any(r.sched != 0 and r.mode == 0 and r.D == 256 for r, _, _ in fused)
    assert any(r.sched != 0 and r.mode == 0 and r.D == 160 for r, _, _ in fused)
    assert any(r.D > 512 for r, _, _ in fused)
    assert any(r.debug & 2 and r.sched == 1 for r, _, _ in fused) and any(r.debug & 4 and r.mode == 0 for r, _, _ in fused)
    assert any(q["chain"] for _, q, _ in fused) and any(q["chain"] for _, q, _ in sep)
    assert {qo["nvol"] for _, _, qo in fused + sep} >= {1, 2, 3, 4, 5}
    assert {r.uniq for r in ROWS} >= {0, 10, 100, 150} and {r.d12 for r in ROWS} >= {-1, 0, 1, 100000}
    assert {r.speckle for r in ROWS} == {0, 1} and {r.sched for r in ROWS} == {0, 1, 2}
    assert {r.D for r in ROWS} >= {16, 32, 48, 64, 128, 160, 256, 512, 1024}


def test_both_options_on_all_four_maps_exact():
    r = BASE[2]
    a, b = _pair(r, 9200)
    p = _params(r)
    want, t = _oracle(r, a, b, p)
    raw, fin = _reference(r, t, p)
    minX1 = r.W - t["S"].shape[1] + min(r.minD, 0)
    craw = CR.conf_raw(t["S"], r.W, minX1)
    out, eng = _run(r, a, b, p, True, conf=1)
    assert np.array_equal(out["disp"], want)
    assert np.array_equal(out["right_raw"], raw) and np.array_equal(out["right"], fin)
    assert np.array_equal(eng.tap(_lib.SGM_TAP_CONF_RAW, r.H, r.W), craw)
    assert np.array_equal(eng.tap(_lib.SGM_TAP_CONF, r.H, r.W), CR.conf_final(craw, want, r.minD))
    assert out["stages"].index("conf") < out["stages"].index("right_wta")


# ---- the device binding ------------------------------------------------------------------------------------------------------
def _resident(pairs, H, W):
    import torch
    dev = torch.device("cuda", 0)
    dl = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a, _ in pairs]
    dr = [torch.from_numpy(np.ascontiguousarray(b)).to(dev) for _, b in pairs]
    dd = [torch.full((H, W), -7, dtype=torch.int16, device=dev) for _ in pairs]
    dm = [torch.full((H, W), 0x5EEE, dtype=torch.int16, device=dev) for _ in pairs]
    torch.cuda.synchronize()
    return dl, dr, dd, dm


ptr = lambda ts: [t.data_ptr() for t in ts]


def _single(p, a, b, H, W, sched=1):
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, sched)
    eng.set_option(_lib.SGM_OPT_RIGHT_VIEW, 1)
    d = eng.compute_host(a, b)
    return d, eng.tap(_lib.SGM_TAP_RIGHT, H, W)


def test_binding_of_the_single_pair_entries_is_consumed_by_one_call():
    H, W, D = 40, 300, 128
    p = U.params(D, 5, 0, 1, speckleWindowSize=30, speckleRange=2)
    pairs = [synth.make_pair(H, W, D, 9300)[:2]]
    want_d, t = O.sgbm_compute(*pairs[0], taps=True, **p)
    raw, want_m = RR.right_view(t["S"], W, W - t["S"].shape[1], p)
    assert (want_m != -16).any()
    dl, dr, dd, dm = _resident(pairs, H, W)
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_RIGHT_VIEW, 1)
    for entry in ("compute", "pipeline"):
        dm[0].fill_(0x5EEE)
        if entry == "compute":
            eng.compute_device(dl[0].data_ptr(), dr[0].data_ptr(), H, W, W, dd[0].data_ptr(), d_rmap=dm[0].data_ptr())
        else:
            eng.pipeline_device(dl[0].data_ptr(), dr[0].data_ptr(), H, W, W, None, dd[0].data_ptr(), None, None, d_rmap=dm[0].data_ptr())
        eng.synchronize()
        assert np.array_equal(dd[0].cpu().numpy(), want_d) and np.array_equal(dm[0].cpu().numpy(), want_m), entry
        # the map went to the bound pointer: the engine's own buffer does not hold it, right_raw is there
        with pytest.raises(cv.error, match="bound"):
            eng.tap(_lib.SGM_TAP_RIGHT, H, W)
        assert np.array_equal(eng.tap(_lib.SGM_TAP_RIGHT_RAW, H, W), raw)
        # consumed: the next call without a new binding writes nothing there, and its map is in the engine again
        dm[0].fill_(0x5A5A)
        eng.compute_device(dl[0].data_ptr(), dr[0].data_ptr(), H, W, W, dd[0].data_ptr())
        eng.synchronize()
        assert (dm[0].cpu().numpy() == 0x5A5A).all(), entry
        assert np.array_equal(eng.tap(_lib.SGM_TAP_RIGHT, H, W), want_m)


@pytest.mark.parametrize("sched,gmax", [(1, 0), (2, 0), (2, 3)])
def test_binding_of_the_batch_entry(sched, gmax):
    """5 pairs: pair after pair (schedule 1), one chained group of 5, groups of 3 + 2 -- each pair's map equals the
    single-pair result for that pair; a second call without a binding leaves the sentinel alone"""
    H, W, D, N = 40, 300, 128, 5
    p = U.params(D, 5, 0, 1, speckleWindowSize=30, speckleRange=2)
    pairs = [synth.make_pair(H, W, D, 9400 + i)[:2] for i in range(N)]
    singles = [_single(p, a, b, H, W, sched) for a, b in pairs]
    _, t = O.sgbm_compute(*pairs[0], taps=True, **p)
    assert np.array_equal(singles[0][1], RR.right_view(t["S"], W, W - t["S"].shape[1], p)[1])
    dl, dr, dd, dm = _resident(pairs, H, W)
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, sched)
    eng.set_option(_lib.SGM_OPT_SWEEP_ROWS, 4)
    eng.set_option(_lib.SGM_OPT_GROUP_MAX, gmax)
    eng.set_option(_lib.SGM_OPT_RIGHT_VIEW, 1)
    eng.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, None, ptr(dd), d_rmaps=ptr(dm))
    eng.synchronize()
    for i in range(N):
        assert np.array_equal(dd[i].cpu().numpy(), singles[i][0]), i
        assert np.array_equal(dm[i].cpu().numpy(), singles[i][1]), (i, int((dm[i].cpu().numpy() != singles[i][1]).sum()))
    assert len({s[1].tobytes() for s in singles}) == N                     # five different maps
    for m in dm:
        m.fill_(0x5A5A)
    eng.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, None, ptr(dd))
    eng.synchronize()
    assert all((m.cpu().numpy() == 0x5A5A).all() for m in dm)
    assert all(np.array_equal(dd[i].cpu().numpy(), singles[i][0]) for i in range(N))


def test_binding_error_returns_and_tap_errors():
    H, W, D = 40, 300, 64
    p = U.params(D, 5, 0, 0, speckleWindowSize=30, speckleRange=2)
    pairs = [synth.make_pair(H, W, D, 9500 + i)[:2] for i in range(3)]
    dl, dr, dd, dm = _resident(pairs, H, W)
    eng = Engine(p)
    with pytest.raises(cv.error, match="SGM_OPT_RIGHT_VIEW"):               # option off
        eng.bind_right_device(ptr(dm[:1]))
    with pytest.raises(cv.error, match="SGM_OPT_RIGHT_VIEW 2"):             # values other than 0 and 1
        eng.set_option(_lib.SGM_OPT_RIGHT_VIEW, 2)
    with pytest.raises(cv.error):
        eng.set_option(_lib.SGM_OPT_RIGHT_VIEW, -1)
    # the taps after an option-off compute
    want0 = O.sgbm_compute(*pairs[0], **p)
    assert np.array_equal(eng.compute_host(*pairs[0]), want0)
    for tap in (_lib.SGM_TAP_RIGHT_RAW, _lib.SGM_TAP_RIGHT):
        with pytest.raises(cv.error, match="SGM_OPT_RIGHT_VIEW"):
            eng.tap(tap, H, W)
    eng.set_option(_lib.SGM_OPT_RIGHT_VIEW, 1)
    with pytest.raises(cv.error, match="SGM_OPT_RIGHT_VIEW"):               # switching it on makes no map: the last compute had none
        eng.tap(_lib.SGM_TAP_RIGHT, H, W)
    with pytest.raises(cv.error, match="pair 1"):                           # a null pointer
        eng.bind_right_device([dm[0].data_ptr(), 0, dm[2].data_ptr()])
    # N differs from the call's pair count: reported by the image call, which consumes the binding all the same
    eng.bind_right_device(ptr(dm[:2]))
    with pytest.raises(cv.error, match="bound 2 maps"):
        eng.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, None, ptr(dd))
    eng.bind_right_device(ptr(dm))
    with pytest.raises(cv.error, match="bound 3 maps"):
        eng.compute_device(dl[0].data_ptr(), dr[0].data_ptr(), H, W, W, dd[0].data_ptr())
    # a failing image call consumes it too (stride smaller than a row), and N = 0 clears one
    eng.bind_right_device(ptr(dm[:1]))
    with pytest.raises(cv.error, match="stride"):
        eng.compute_device(dl[0].data_ptr(), dr[0].data_ptr(), H, W, W - 1, dd[0].data_ptr())
    eng.bind_right_device(ptr(dm[:1]))
    eng.bind_right_device([])
    for m in dm:
        m.fill_(0x5A5A)
    eng.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, None, ptr(dd))     # the engine is usable, nothing is bound
    eng.synchronize()
    assert all((m.cpu().numpy() == 0x5A5A).all() for m in dm)
    assert np.array_equal(dd[2].cpu().numpy(), O.sgbm_compute(*pairs[2], **p))
    # the host batch entry computes as before with the option on (no per-pair right map from it)
    disps = eng.compute_batch_host(np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]))
    assert all(np.array_equal(disps[i], O.sgbm_compute(*pairs[i], **p)) for i in range(3))


# ---- the Python surface ----------------------------------------------------------------------------------------------------
def test_compute_left_right_and_the_cached_engine():
    import torch
    H, W, D = 40, 300, 64
    p = U.params(D, 5, 0, 0, speckleWindowSize=30, speckleRange=2)
    a, b, _ = synth.make_pair(H, W, D, 9600)
    want, t = O.sgbm_compute(a, b, taps=True, **p)
    _, fin = RR.right_view(t["S"], W, W - t["S"].shape[1], p)
    m = cv.StereoSGBM_create(**p)
    d, rm = m.computeLeftRight(a, b)
    assert isinstance(rm, np.ndarray) and rm.dtype == np.int16 and rm.shape == (H, W)
    assert np.array_equal(d, want) and np.array_equal(rm, fin)
    # the cached engine is back to not producing the map: plain compute() does not pay for it
    eng = cv.get_engine(p)
    eng.set_option(_lib.SGM_OPT_PROFILE, 1)
    assert np.array_equal(m.compute(a, b), want)
    names = [n for n, _, _ in eng.stage_times()]
    assert not [n for n in names if n.startswith("right_")], names
    with pytest.raises(cv.error, match="SGM_OPT_RIGHT_VIEW"):
        eng.tap(_lib.SGM_TAP_RIGHT, H, W)
    eng.set_option(_lib.SGM_OPT_PROFILE, 0)
    # HIP tensors in, tensors out; a colour pair through the same validation
    dev = torch.device("cuda", 0)
    dt, rt = m.computeLeftRight(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
    assert rt.dtype == torch.int16 and rt.is_cuda and np.array_equal(dt.cpu().numpy(), want) and np.array_equal(rt.cpu().numpy(), fin)
    assert np.array_equal(m.compute(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)).cpu().numpy(), want)
    L3, R3 = BC.colour_pair(30, 260, 32, seed=9601)
    p3 = U.params(32, 3, 0, 1, penalty="plain", speckleWindowSize=30, speckleRange=2)
    w3, t3 = V.sgbm_compute(L3, R3, taps=True, **p3)
    d3, r3 = cv.StereoSGBM_create(**p3).computeLeftRight(L3, R3)
    assert np.array_equal(d3, w3) and np.array_equal(r3, RR.right_view(t3["S"], 260, 260 - t3["S"].shape[1], p3)[1])
    with pytest.raises(cv.error):
        m.computeLeftRight(a, b[:, :-1])


# ---- history, guarded buffers ------------------------------------------------------------------------------------------------
def test_one_engine_alternating_option_shapes_and_modes_then_from_poisoned_buffers():
    shapes = [(60, 420, 1), (24, 200, 0), (60, 420, 1), (33, 310, 3), (20, 70, 0)]
    cases = []
    for i, (H, W, mode) in enumerate(shapes):
        p = U.params(64, 5, 0, mode, speckleWindowSize=30, speckleRange=2)
        a, b, _ = synth.make_pair(H, W, 64, 9700 + i)
        want, t = (V if mode == 3 else O).sgbm_compute(a, b, taps=True, **p)
        cases.append((p, a, b, want) + tuple(RR.right_view(t["S"], W, W - t["S"].shape[1], p)))
    engines = {}
    try:
        for rnd in range(2):
            for i, (p, a, b, want, raw, fin) in enumerate(cases):
                eng = engines.setdefault(p["mode"], Engine(p))      # (the mode is an argument of sgm_create: one engine per mode)
                if rnd == 1:
                    eng.set_option(_lib.SGM_OPT_POISON, 0xA5)
                for on in (1, 0, 1):
                    eng.set_option(_lib.SGM_OPT_RIGHT_VIEW, on)
                    assert np.array_equal(eng.compute_host(a, b), want), (rnd, i, on)
                    if on:
                        assert np.array_equal(eng.tap(_lib.SGM_TAP_RIGHT_RAW, *a.shape), raw), (rnd, i)
                        assert np.array_equal(eng.tap(_lib.SGM_TAP_RIGHT, *a.shape), fin), (rnd, i)
                    else:
                        with pytest.raises(cv.error, match="SGM_OPT_RIGHT_VIEW"):
                            eng.tap(_lib.SGM_TAP_RIGHT, *a.shape)
                    if rnd == 1:
                        eng.set_option(_lib.SGM_OPT_POISON, 0xA5)
    finally:
        for eng in engines.values():
            eng.set_option(_lib.SGM_OPT_POISON, -1)


def test_right_view_rows_with_every_buffer_guarded():
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "right_view_guard_child.py")], capture_output=True, text=True,
                       env=env, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"RIGHT_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) == 5, tail


# ---- full size ---------------------------------------------------------------------------------------------------------------
def test_4k_d256_hh_against_the_reference_on_the_oracles_volume():
    H, W, D = 2160, 3840, 256
    p = U.params(D, 7, 0, 1)
    a, b, _ = synth.make_pair(H, W, D, 9800)
    ws = O.workspace(H, W, **p)
    want = O.sgbm_compute(a, b, workspace=ws, **p)
    raw, fin = RR.right_view(ws["S"], W, W - ws["S"].shape[1], p)
    del ws
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_RIGHT_VIEW, 1)
    got = eng.compute_host(a, b)
    assert eng.headroom()["ok"]
    assert np.array_equal(got, want)
    g = eng.tap(_lib.SGM_TAP_RIGHT_RAW, H, W)
    assert np.array_equal(g, raw), U.describe_mismatch("right_raw", g, raw)
    g = eng.tap(_lib.SGM_TAP_RIGHT, H, W)
    assert np.array_equal(g, fin), U.describe_mismatch("right", g, fin)
    assert (fin != -16).mean() > 0.5


def test_1080p_d128_sgbm_batch_of_four_through_the_binding():
    H, W, D, N = 1080, 1920, 128, 4
    p = U.params(D, 5, 0, 0)
    pairs = [synth.make_pair(H, W, D, 9900 + i)[:2] for i in range(N)]
    dl, dr, dd, dm = _resident(pairs, H, W)
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, 2)
    eng.set_option(_lib.SGM_OPT_RIGHT_VIEW, 1)
    eng.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, None, ptr(dd), d_rmaps=ptr(dm))
    eng.synchronize()
    assert eng.headroom()["ok"]
    for i, (a, b) in enumerate(pairs):
        want, t = O.sgbm_compute(a, b, taps=True, **p)
        assert t["headroom_ok"]
        _, fin = RR.right_view(t["S"], W, W - t["S"].shape[1], p)
        del t
        assert np.array_equal(dd[i].cpu().numpy(), want), i
        got = dm[i].cpu().numpy()
        assert np.array_equal(got, fin), (i, U.describe_mismatch("right", got, fin))
