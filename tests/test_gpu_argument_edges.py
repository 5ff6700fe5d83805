"""The engine against the C oracle at the argument edges of argument_edges.py (needs an MI355X): preFilterCap above 127
(ftzero >= 129, whose prefilter values are bytes), even / non-positive block sizes, non-positive and
inverted penalties, negative uniquenessRatio / disp12MaxDiff, minDisparity far from 0, fully saturated S vectors and
the speckle switches -- every stage tap and the headroom record, on all three schedules.  Then the same caps for
NP = 2 and 4 and on the colour path, and reprojection with a dense Q."""
import numpy as np
import pytest
import torch

import argument_edges as E
import bruteforce_color as BC
import bruteforce_sgbm as B
import parity_util as U
from oracle import oracle as O
from stereo_reconstruction_cv_amd import _lib
from stereo_reconstruction_cv_amd import stereo as cv
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu

TAPS = ("C", "S", "disp_raw", "disp_median", "disp")


def _schedule_options(schedule, k):
    """the option values test_gpu_fuzz.py gives schedule `schedule` for case index k.  A deliberate copy: the fuzz keeps
    its tables inline and stays as it is, and these cases need not follow it if it changes -- any value of each option is
    a valid setting that must give the same taps."""
    return dict(sweep_rows=([0, 1, 2, 4][k % 4] if schedule == 1 else [1, 2, 3, 5][k % 4]) if schedule else 0,
                prepass_rows=[0, 3, 11, 0, 64][k % 5] if schedule == 1 else 0,
                chain_wgs=[0, 1, 2, 7][k % 4] if schedule == 2 else 0)


def _check_all_schedules(l, r, p, k):
    """every tap and the headroom record on schedules 1, 0 and 2 against the oracle; a case outside the int16 regime
    must be reported as such by the engine (no parity is claimed there)"""
    want, t = O.sgbm_compute(l, r, taps=True, **p)
    t["disp"] = want
    for schedule in (1, 0, 2):
        h = U.run_hip_with_taps(l, r, p, schedule=schedule, **_schedule_options(schedule, k))
        if not t["headroom_ok"]:
            assert not h["headroom"]["ok"], (schedule, h["headroom"], t["max_cost_plus_p2"], t["max_delta"])
            continue
        bad = [U.describe_mismatch(n, h[n], t[n]) for n in TAPS if n in h and n in t and not np.array_equal(h[n], t[n])]
        if not U.headroom_equal(h, t):
            bad.append(f"headroom record: hip {h['headroom']} oracle {t['max_cost_plus_p2']}, {t['max_delta']}")
        assert not bad, f"schedule {schedule} {p} {l.shape}\n" + "\n".join(bad)
    return t


@pytest.mark.parametrize("k,name", list(enumerate(E.EDGES)))
def test_edge_bit_exact(k, name):
    l, r, p = E.edge_case(name)
    t = _check_all_schedules(l, r, p, k)
    assert t["headroom_ok"]


@pytest.mark.parametrize("seed", range(48))
def test_random_edges_bit_exact(seed):
    l, r, p = E.random_case(seed)
    _check_all_schedules(l, r, p, seed)


# NP = 2 (D 129 .. 256) and NP = 4 (D 257 .. 512) lane packings at the caps that wrap, and a case outside the regime
WIDE = {  # name: (H, W, D, minD, bs, mode, cap, noise)
    "np2_cap128": (9, 260, 192, 0, 5, 1, 128, False),
    "np2_cap200_mind_neg": (8, 330, 256, -40, 3, 0, 200, False),
    "np2_cap1000_noise": (7, 300, 256, 0, 3, 1, 1000, True),
    "np2_cap300_mind_plus_d_neg": (6, 420, 144, -170, 3, 0, 300, False),
    "np4_cap128": (6, 400, 320, 0, 3, 0, 128, False),
    "np4_cap200_mind_pos": (6, 600, 512, 30, 5, 1, 200, False),
    "np4_cap1000": (5, 560, 448, -5, 3, 1, 1000, False),
    "np1_cap1000_out_of_regime": (10, 120, 64, 0, 21, 1, 1000, True),
}


@pytest.mark.parametrize("k,name", list(enumerate(WIDE)))
def test_wide_disparity_ranges_at_large_caps(k, name):
    H, W, D, minD, bs, mode, cap, noise = WIDE[name]
    p = E.edge_params(D, bs, minD=minD, mode=mode, cap=cap)
    l, r = E.pair(H, W, D, 300 + k, noise)
    t = _check_all_schedules(l, r, p, k)
    assert t["headroom_ok"] == (not name.endswith("out_of_regime"))


# ---- colour path (SGM_OPT_CHANNELS = 3) at the caps that wrap ---------------------------------------------------------
COLOUR = [  # H, W, D, minD, bs, mode, cap, schedule, sweep_rows, chain_wgs
    (12, 90, 32, 0, 3, 1, 128, 1, 0, 0),
    (11, 100, 48, -3, 5, 0, 200, 0, 0, 0),
    (12, 96, 32, 2, 3, 1, 1000, 2, 3, 2),
    (10, 300, 192, 0, 3, 0, 1000, 1, 3, 0),          # NP = 2
]


@pytest.mark.parametrize("H,W,D,minD,bs,mode,cap,schedule,rows,wgs", COLOUR)
def test_colour_at_large_caps(H, W, D, minD, bs, mode, cap, schedule, rows, wgs):
    p = E.edge_params(D, bs, minD=minD, mode=mode, cap=cap, spw=12, spr=2)
    L3, R3 = BC.colour_pair(H, W, D, seed=5 * H + D + cap, minD=minD)
    want = BC.sgbm_c3(L3, R3, **p)
    # the colour cost is the sum of the oracle's three channel costs (which wrap mod 256 at these caps)
    Csum = sum(O.sgbm_compute(np.ascontiguousarray(L3[..., c]), np.ascontiguousarray(R3[..., c]), taps=True, **p)[1]["C"]
               .astype(np.int32) for c in range(3))
    assert np.array_equal(Csum, want["C"])
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_KEEP_AGGR, 1)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, schedule)
    eng.set_option(_lib.SGM_OPT_SWEEP_ROWS, rows)
    if wgs:
        eng.set_option(_lib.SGM_OPT_CHAIN_WGS, wgs)
    got = eng.compute_host(L3, R3)
    hr = eng.headroom()
    assert hr["ok"] and int(want["C"].max()) + p["P2"] <= hr["max_cost_plus_p2"] <= 32767, hr
    assert hr["max_delta"] <= 32767
    bad = [U.describe_mismatch(n, eng.tap(tap, H, W), want[n]) for n, tap in
           (("C", _lib.SGM_TAP_COST), ("S", _lib.SGM_TAP_AGGR), ("disp_raw", _lib.SGM_TAP_DISP_RAW),
            ("disp_median", _lib.SGM_TAP_DISP_MEDIAN)) if not np.array_equal(eng.tap(tap, H, W), want[n])]
    if not np.array_equal(got, want["disp"]):
        bad.append(U.describe_mismatch("disp", got, want["disp"]))
    assert not bad, "\n".join(bad)
    assert (got > (minD - 1) * 16).mean() > 0.2


# ---- reprojection with a dense Q ---------------------------------------------------------------------------------------
def _exact(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _shows_contraction(d, Q, pins, hm=False):
    """the pinned components are 0 in Appendix B's arithmetic and not 0 with contracted multiply-adds (the case can
    tell a build that lost -ffp-contract=off from a correct one)"""
    plain, fused = B.reproject(d, Q, hm), B.reproject(d, Q, hm, fused=True)
    return all(plain[y, x, r] == 0 and fused[y, x, r] != 0 for r, (y, x) in enumerate(pins)) and not _exact(plain, fused)


@pytest.mark.parametrize("hm", [False, True])
def test_reproject_dense_Q(hm):
    """every Q entry non-trivial and Q[3][3] != 0, on a map with W == 0 exactly at many pixels and rows pinned where
    contraction shows: bit for bit against the oracle and the restatement, the signs of inf included, through the host
    entry and a HIP tensor (k_reproject)"""
    d = E.dense_Q_disparity()
    Q, pins = E.pin_xyz_rows(E.dense_Q(), d)
    assert (E.w_of(Q, d) == 0).sum() >= 30 and _shows_contraction(d, Q, pins, hm)
    want = O.reproject(d, Q, hm)
    assert _exact(want, B.reproject(d, Q, hm)) and np.isinf(want).any()
    assert _exact(cv.reprojectImageTo3D(d, Q, handleMissingValues=hm), want)
    got = cv.reprojectImageTo3D(torch.from_numpy(d).cuda(), Q, handleMissingValues=hm)
    assert _exact(got.cpu().numpy(), want)


def test_batch_fused_reproject_dense_Q():
    """the batch entry's fused float conversion + reprojection (k_float_xyz) with a dense Q chosen on the first computed
    map: W exactly 0 at one of its pixels, and X, Y and Z pinned where contraction shows"""
    H, W, D = 24, 140, 32
    p = E.edge_params(D, 5, mode=1)
    pairs = [E.pair(H, W, D, 500 + i, False) for i in range(3)]
    f0 = O.disp_to_float(O.sgbm_compute(*pairs[0], **p))
    Q = E.dense_Q()
    y0, x0 = np.argwhere(f0 > 0)[len(np.argwhere(f0 > 0)) // 2]
    Q[3, 3] = -((Q[3, 0] * x0 + Q[3, 1] * y0) + Q[3, 2] * float(f0[y0, x0]))     # dyadic: the sum is exactly 0 there
    assert Q[3, 3] != 0
    Q, pins = E.pin_xyz_rows(Q, f0)
    assert _shows_contraction(f0, Q, pins)
    eng = Engine(p)
    disps, xyz = eng.compute_batch_host(np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]), Q)
    zeros = 0
    for i, (a, b) in enumerate(pairs):
        assert np.array_equal(disps[i], O.sgbm_compute(a, b, **p)), i
        f = O.disp_to_float(disps[i])
        w_zero = E.w_of(Q, f) == 0
        zeros += int(w_zero.sum())
        want = O.reproject(f, Q)
        assert _exact(want, B.reproject(f, Q))
        assert _exact(xyz[i], want), i
        assert not np.isfinite(xyz[i][w_zero]).any()
    assert zeros >= 1
