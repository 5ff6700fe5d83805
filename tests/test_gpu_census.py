"""The census matching cost on the device (needs an MI355X): SGM_OPT_COST = SGM_COST_CENSUS, StereoSGBM.setCostFunction.

Yardstick: tests/census_ref.py -- the definition of include/sgm_hip.h in numpy, composed with the stage functions of
tests/bruteforce_sgbm.py; tests/test_census_reference.py ties it to answers worked out by hand.  Every comparison is exact.
Which box route a row takes (k_box_u8, or k_hsum_u8 + k_vsum*) is read from the profiled compute, not assumed."""
import os
import re
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

import census_ref as CE
import confidence_ref as CR
import parity_util as U
import right_view_ref as RV
from oracle import oracle as O
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd import stereo as cv
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS = _lib.SGM_COST_CENSUS


def _engine(p, cost=CENSUS, sched=1, debug=0, keep=False, profile=False, **opts):
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_COST, cost)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, sched)
    if debug:
        eng.set_option(_lib.SGM_OPT_DEBUG, debug)
    if keep:
        eng.set_option(_lib.SGM_OPT_KEEP_AGGR, 1)
    if profile:
        eng.set_option(_lib.SGM_OPT_PROFILE, 1)
    for k, v in opts.items():
        eng.set_option(getattr(_lib, k), v)
    return eng


def _pair(H, W, D, seed):
    return synth.make_pair(H, W, D, seed)[:2]


# ---- 1. the block cost, every branch ----------------------------------------------------------------------------------------
CRow = namedtuple("CRow", "H W D minD bs debug route")
COST_ROWS = [
    CRow(40, 316, 16, 0, 5, 0, "box"),        # D <= 32: one thread per pixel; k_box_u8 in lane groups, three bands of 16 rows
    CRow(40, 307, 16, -9, 3, 4, "hsum"),      # debug 4: the wave form with 8 of 64 lanes, and the int16 route
    CRow(40, 339, 32, 7, 7, 0, "box"),
    CRow(40, 316, 16, 0, 1, 0, "hsum"),       # the thread-per-pixel form in front of k_hsum_u8 + k_vsum*: blockSize 1 ...
    CRow(23, 341, 32, -9, 13, 0, "hsum"),     # ... and 13 (the generic k_vsum), no debug bit
    CRow(40, 332, 32, 0, 5, 4, "hsum"),
    CRow(41, 357, 48, -9, 5, 0, "box"),       # NP = 1, 24 lanes
    CRow(40, 364, 64, 0, 11, 0, "box"),
    CRow(40, 403, 96, 7, 1, 0, "hsum"),       # blockSize 1: the plain census cost
    CRow(40, 428, 128, 0, 13, 0, "hsum"),     # blockSize 13: no k_box_u8 instantiation, the generic k_vsum
    CRow(40, 437, 128, -9, 5, 0, "box"),      # NP = 1, all 64 lanes
    CRow(40, 460, 160, 0, 5, 256, "hsum"),    # debug 256; NP = 2, 40 lanes
    CRow(40, 563, 256, 7, 3, 0, "box"),
    CRow(40, 556, 256, 0, 7, 256, "hsum"),
    CRow(40, 572, 272, 0, 5, 0, "box"),       # NP = 4, 34 lanes
    CRow(40, 821, 512, -9, 7, 0, "box"),
    CRow(9, 828, 528, 0, 5, 0, "hsum"),       # D > 512: NP = 8, 33 lanes
    CRow(9, 1331, 1024, 7, 3, 0, "hsum"),
    CRow(9, 1324, 1024, 0, 11, 0, "hsum"),
    CRow(5, 400, 128, 0, 7, 0, "box"),        # H below the census window's and the box window's height
    CRow(2, 150, 32, 0, 5, 0, "box"),
    CRow(1, 90, 64, -9, 3, 0, "box"),
    CRow(12, 17, 16, 0, 5, 0, "box"),         # W1 = 1, W far below a block of k_census
    CRow(12, 129, 128, 0, 5, 0, "box"),       # W1 = 1 in the wave form
    CRow(12, 67, 64, 0, 3, 0, "box"),         # W1 = 3
    CRow(12, 257, 128, 0, 5, 0, "box"),       # W1 = 129: a chunk of 128 columns and one of 1
    CRow(12, 513, 256, 0, 5, 0, "box"),       # W1 = 257: 128 + 128 + 1
    CRow(12, 526, 256, 0, 5, 256, "hsum"),    # W1 = 270: 128 + 128 + 14, with a partial last block of the ring loop
    CRow(13, 389, 64, 0, 5, 0, "box"),        # W1 = 325: odd everything
]
crow_id = lambda r: f"{r.H}x{r.W} D{r.D} minD{r.minD} bs{r.bs} dbg{r.debug}"


@pytest.mark.parametrize("r", COST_ROWS, ids=crow_id)
def test_block_cost_equals_the_reference(r):
    a, b = _pair(r.H, r.W, r.D, 100 + r.D + r.bs)
    p = U.params(r.D, r.bs, r.minD, 1, penalty="plain")
    want = CE.block_cost(CE.pixel_cost(a, b, r.minD, r.D), r.bs // 2)
    assert want.shape[1] > 0 and want.max() <= 62 * r.bs * r.bs and want.any()
    eng = _engine(p, debug=r.debug, profile=True)
    eng.compute_host(a, b)
    names = [n for n, _, _ in eng.stage_times()]
    assert names[:2] == ["census", "cost_pix_census"], names
    assert names[2:4] == ["cost_hsum", "cost_vsum"] if r.route == "hsum" else names[2] == "cost_box", names
    assert "cost_box" not in names[3:] and "features" not in names and "cost_pix" not in names, names
    got = eng.tap(_lib.SGM_TAP_COST, r.H, r.W)
    assert got.shape == want.shape
    assert np.array_equal(got, want), U.describe_mismatch("C", got, want)
    # the headroom word of the cost stage comes out right on both box routes (the running-sum intermediate included)
    pix = CE.pixel_cost(a, b, r.minD, r.D)
    assert eng.headroom()["max_cost_plus_p2"] == p["P2"] + CE.max_cost(pix, want, r.bs // 2)


@pytest.mark.parametrize("H,W,D,minD", [(10, 100, 128, 0), (7, 16, 16, -9), (6, 8, 16, 0), (3, 2, 16, 0)])
def test_no_matched_column_gives_the_invalid_map_and_no_fault(H, W, D, minD):
    p = U.params(D, 5, minD, 1)
    a, b = _pair(H, W, D, 55)
    eng = _engine(p)
    assert eng.geometry(W)[1] <= 0
    got = eng.compute_host(a, b)
    assert np.array_equal(got, np.full((H, W), (minD - 1) * 16, np.int16))
    assert eng.tap(_lib.SGM_TAP_COST, H, W).size == 0


# ---- 2. the whole pipeline ---------------------------------------------------------------------------------------------------
PRow = namedtuple("PRow", "H W D minD bs mode sched penalty")
PIPE_ROWS = [
    PRow(40, 300, 16, 0, 5, 0, 1, "notebook"),
    PRow(40, 300, 32, 0, 5, 0, 2, "notebook"),
    PRow(31, 300, 16, 0, 1, 1, 1, "notebook"),
    PRow(40, 300, 64, 0, 5, 1, 1, "notebook"),
    PRow(40, 300, 64, 0, 1, 1, 0, "notebook"),
    PRow(38, 293, 64, 7, 7, 3, 1, "notebook"),
    PRow(40, 300, 128, 0, 5, 0, 1, "notebook"),
    PRow(40, 300, 128, -9, 3, 1, 2, "notebook"),
    PRow(40, 300, 128, 0, 5, 3, 2, "notebook"),
    PRow(33, 300, 128, 0, 13, 0, 2, "plain"),
    PRow(40, 300, 256, 0, 5, 1, 1, "notebook"),
    PRow(40, 300, 256, 0, 5, 1, 2, "notebook"),
    PRow(40, 300, 256, 0, 5, 0, 0, "notebook"),
    PRow(9, 783, 528, 0, 5, 1, 1, "notebook"),
]
prow_id = lambda r: f"{r.H}x{r.W} D{r.D} minD{r.minD} bs{r.bs} mode{r.mode} sched{r.sched}"


@pytest.mark.parametrize("r", PIPE_ROWS, ids=prow_id)
def test_every_stage_equals_the_reference(r):
    a, b = _pair(r.H, r.W, r.D, 200 + r.D + r.mode)
    p = U.params(r.D, r.bs, r.minD, r.mode, penalty=r.penalty, speckleWindowSize=30, speckleRange=2)
    t = CE.census_sgbm(a, b, **p)
    assert t["headroom"]["ok"]
    eng = _engine(p, sched=r.sched, keep=True)
    got = dict(disp=eng.compute_host(a, b), disp_raw=eng.tap(_lib.SGM_TAP_DISP_RAW, r.H, r.W),
               disp_median=eng.tap(_lib.SGM_TAP_DISP_MEDIAN, r.H, r.W), C=eng.tap(_lib.SGM_TAP_COST, r.H, r.W),
               S=eng.tap(_lib.SGM_TAP_AGGR, r.H, r.W))
    for k in ("C", "S", "disp_raw", "disp_median", "disp"):
        assert np.array_equal(got[k], t[k]), U.describe_mismatch(k, got[k], t[k])
    assert eng.headroom() == t["headroom"]
    assert (t["disp"] != (r.minD - 1) * 16).mean() > 0.05          # not a degenerate row


# ---- 3. invariance on the device ----------------------------------------------------------------------------------------------
def test_disparity_is_invariant_under_increasing_intensity_maps_and_bt_is_not():
    H, W, D = 203, 700, 128
    a, b = _pair(H, W, D, 303)
    a, b = np.minimum(a, 225), np.minimum(b, 225)
    assert a.max() <= 225 and b.max() <= 225
    f = lambda v: (v + 30).astype(np.uint8)
    g = lambda v: (v + 30 * (v >= 128)).astype(np.uint8)
    p = U.params(D, 5, 0, 1)
    eng = _engine(p)
    base = eng.compute_host(a, b)
    assert (base != -16).mean() > 0.3
    for m in (f, g):
        assert np.array_equal(eng.compute_host(a, m(b)), base)
        assert np.array_equal(eng.compute_host(m(a), b), base)
    eng.set_option(_lib.SGM_OPT_COST, _lib.SGM_COST_BT)
    bt = eng.compute_host(a, b)
    assert np.array_equal(bt, O.sgbm_compute(a, b, **p))
    assert not (np.array_equal(eng.compute_host(a, f(b)), bt) and np.array_equal(eng.compute_host(g(a), b), bt))


# ---- 4. the optional maps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,D,minD,mode,sched", [(40, 300, 128, 0, 1, 1), (31, 333, 64, -3, 0, 2)])
def test_confidence_with_census(H, W, D, minD, mode, sched):
    a, b = _pair(H, W, D, 400 + D)
    p = U.params(D, 5, minD, mode, speckleWindowSize=30, speckleRange=2)
    t = CE.census_sgbm(a, b, **p)
    raw = CR.conf_raw(t["S"].astype(np.int16), W, t["minX1"])
    eng = _engine(p, sched=sched, SGM_OPT_CONFIDENCE=1)
    got = eng.compute_host(a, b)
    assert np.array_equal(got, t["disp"])
    assert np.array_equal(eng.tap(_lib.SGM_TAP_CONF_RAW, H, W), raw)
    assert np.array_equal(eng.tap(_lib.SGM_TAP_CONF, H, W), CR.conf_final(raw, t["disp"], minD))
    assert CR.deciles_populated(raw) >= 5


@pytest.mark.parametrize("H,W,D,minD,mode,sched", [(40, 300, 128, 0, 1, 1), (31, 333, 64, -3, 0, 2)])
def test_right_view_with_census(H, W, D, minD, mode, sched):
    a, b = _pair(H, W, D, 450 + D)
    p = U.params(D, 5, minD, mode, speckleWindowSize=30, speckleRange=2)
    t = CE.census_sgbm(a, b, **p)
    raw, fin = RV.right_view(t["S"].astype(np.int16), W, t["minX1"], p)
    eng = _engine(p, sched=sched, SGM_OPT_RIGHT_VIEW=1)
    got = eng.compute_host(a, b)
    assert np.array_equal(got, t["disp"])
    assert np.array_equal(eng.tap(_lib.SGM_TAP_RIGHT_RAW, H, W), raw)
    assert np.array_equal(eng.tap(_lib.SGM_TAP_RIGHT, H, W), fin)
    assert (fin != (minD - 1) * 16).mean() > 0.05


# ---- 5. history ---------------------------------------------------------------------------------------------------------------
def test_one_engine_alternating_cost_and_shapes_then_from_poisoned_buffers():
    p = U.params(64, 5, 0, 1, speckleWindowSize=30, speckleRange=2)
    cases = []
    for i, (H, W) in enumerate([(60, 420), (24, 200), (60, 420), (33, 310)]):
        a, b = _pair(H, W, 64, 500 + i)
        cases.append((a, b, O.sgbm_compute(a, b, **p), CE.census_sgbm(a, b, **p)["disp"]))
    eng = Engine(p)
    try:
        for rnd in range(2):
            if rnd == 1:
                eng.set_option(_lib.SGM_OPT_POISON, 0xA5)
            for i, (a, b, bt, census) in enumerate(cases):
                for cost in (1, 0, 1, 0):
                    eng.set_option(_lib.SGM_OPT_COST, cost)
                    got = eng.compute_host(a, b)
                    assert np.array_equal(got, census if cost else bt), (rnd, i, cost)
                    if rnd == 1:
                        eng.set_option(_lib.SGM_OPT_POISON, 0xA5)
    finally:
        eng.set_option(_lib.SGM_OPT_POISON, -1)


# ---- 6. the batch entries -----------------------------------------------------------------------------------------------------
def test_batch_entries_equal_the_single_pair_results():
    import torch
    H, W, D, N = 40, 300, 128, 3
    p = U.params(D, 5, 0, 1, speckleWindowSize=30, speckleRange=2)
    pairs = [_pair(H, W, D, 600 + i) for i in range(N)]
    single = [_engine(p).compute_host(a, b) for a, b in pairs]
    assert np.array_equal(single[0], CE.census_sgbm(*pairs[0], **p)["disp"])
    assert not np.array_equal(single[0], O.sgbm_compute(*pairs[0], **p))
    dev = torch.device("cuda", 0)
    dl = [torch.from_numpy(a).to(dev) for a, _ in pairs]
    dr = [torch.from_numpy(b).to(dev) for _, b in pairs]
    dd = [torch.full((H, W), -7, dtype=torch.int16, device=dev) for _ in pairs]
    torch.cuda.synchronize()
    ptr = lambda ts: [t.data_ptr() for t in ts]
    eng = _engine(p, sched=2, SGM_OPT_GROUP_MAX=2)
    eng.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, None, ptr(dd))
    eng.synchronize()
    assert eng.headroom()["ok"]
    for i in range(N):
        assert np.array_equal(dd[i].cpu().numpy(), single[i]), i
    lefts, rights = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    for sched in (1, 2):
        disps = _engine(p, sched=sched).compute_batch_host(lefts, rights)
        for i in range(N):
            assert np.array_equal(disps[i], single[i]), (sched, i)


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------
def test_bad_option_value_and_colour_census_are_refused_and_the_engine_stays_usable():
    H, W, D = 30, 260, 32
    p = U.params(D, 5, 0, 1)
    a, b = _pair(H, W, D, 700)
    eng = Engine(p)
    L = _lib.load()
    for bad in (2, -1):
        assert L.sgm_set_option(eng._h, _lib.SGM_OPT_COST, bad) == -1            # SGM_ERR_INVALID_ARG
        assert "SGM_OPT_COST" in _lib.last_error()
    assert np.array_equal(eng.compute_host(a, b), O.sgbm_compute(a, b, **p))     # the refused values changed nothing
    eng.set_option(_lib.SGM_OPT_COST, CENSUS)
    want = CE.census_sgbm(a, b, **p)["disp"]
    assert np.array_equal(eng.compute_host(a, b), want)
    a3, b3 = np.stack([a] * 3, axis=-1), np.stack([b] * 3, axis=-1)
    disp = np.empty((H, W), np.int16)
    eng.set_option(_lib.SGM_OPT_CHANNELS, 3)
    assert L.sgm_compute(eng._h, a3.ctypes.data, b3.ctypes.data, H, W, 3 * W, disp.ctypes.data) == -4   # SGM_ERR_UNSUPPORTED
    assert "SGM_COST_CENSUS" in _lib.last_error()
    with pytest.raises(cv.error, match="SGM_COST_CENSUS"):
        eng.compute_batch_host(np.stack([a3, a3]), np.stack([b3, b3]))
    assert np.array_equal(eng.compute_host(a, b), want)                          # (compute_host sets the channels back to 1)
    eng.set_option(_lib.SGM_OPT_COST, _lib.SGM_COST_BT)
    assert np.array_equal(eng.compute_host(a3, b3).shape, (H, W))                # colour under BT still runs


# ---- 8. Python ----------------------------------------------------------------------------------------------------------------
def test_two_matchers_sharing_a_cached_engine_each_get_their_own_cost():
    import torch
    H, W, D = 40, 300, 64
    p = U.params(D, 5, 0, 1, speckleWindowSize=30, speckleRange=2)
    a, b = _pair(H, W, D, 800)
    t = CE.census_sgbm(a, b, **p)
    bt = O.sgbm_compute(a, b, **p)
    assert not np.array_equal(bt, t["disp"])
    cv.clear_engine_cache()
    m_bt = cv.StereoSGBM_create(**p)
    m_ce = cv.StereoSGBM_create(**p, costFunction=cv.STEREO_COST_CENSUS)
    dev = torch.device("cuda", 0)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    for _ in range(2):
        assert np.array_equal(m_ce.compute(a, b), t["disp"])
        assert np.array_equal(m_bt.compute(a, b), bt)
        assert np.array_equal(m_ce.compute(ta, tb).cpu().numpy(), t["disp"])
        assert np.array_equal(m_bt.compute(ta, tb).cpu().numpy(), bt)
    assert len(cv._engine_cache) == 1                       # one engine served both
    # ... and the census matcher leaves it as get_engine() hands it out to everyone else: at the default cost
    assert np.array_equal(m_ce.compute(a, b), t["disp"])
    assert np.array_equal(cv.get_engine(p).compute_host(a, b), bt)
    assert np.array_equal(m_ce.compute(ta, tb).cpu().numpy(), t["disp"])
    assert np.array_equal(cv.get_engine(p).compute_host(a, b), bt)
    raw = CR.conf_raw(t["S"].astype(np.int16), W, t["minX1"])
    d, c = m_ce.computeWithConfidence(a, b)
    assert np.array_equal(d, t["disp"]) and np.array_equal(c, CR.conf_final(raw, t["disp"], 0))
    assert np.array_equal(m_bt.computeWithConfidence(a, b)[0], bt)
    d, r = m_ce.computeLeftRight(ta, tb)
    assert np.array_equal(d.cpu().numpy(), t["disp"])
    assert np.array_equal(r.cpu().numpy(), RV.right_view(t["S"].astype(np.int16), W, t["minX1"], p)[1])
    m_bt.setCostFunction(cv.STEREO_COST_CENSUS)
    assert np.array_equal(m_bt.compute(a, b), t["disp"])
    with pytest.raises(cv.error, match="single-channel"):
        m_ce.compute(np.stack([a] * 3, axis=-1), np.stack([b] * 3, axis=-1))


# ---- 9. guarded buffers -------------------------------------------------------------------------------------------------------
def test_census_rows_with_every_buffer_guarded():
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "census_guard_child.py")], capture_output=True, text=True,
                       env=env, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"CENSUS_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) == 7, tail


# ---- 10. full size ------------------------------------------------------------------------------------------------------------
def test_4k_d256_hh_cost_rows_headroom_and_invariance():
    """3840 x 2160, D = 256, blockSize 5, MODE_HH.  The block cost of the first, some middle and the last rows -- whose
    offsets in the volume lie past 2^31 bytes -- against the reference computed for just those rows.
    Not covered: the int16 route that byte volumes from 2 GiB take (4K D = 512) at its real size."""
    H, W, D, r = 2160, 3840, 256, 2
    p = U.params(D, 5, 0, 1)
    a, b = _pair(H, W, D, 1000)
    a, b = np.minimum(a, 225), np.minimum(b, 225)
    eng = _engine(p)
    base = eng.compute_host(a, b)
    assert eng.headroom()["ok"]
    C = eng.tap(_lib.SGM_TAP_COST, H, W)
    assert C.nbytes > 1 << 31
    for rows in (np.arange(0, 8), np.arange(1080, 1096), np.arange(H - 8, H)):
        need = np.arange(max(rows[0] - r, 0), min(rows[-1] + r, H - 1) + 1)
        pix = CE.pixel_cost(a, b, 0, D, rows=need)
        xs = np.arange(pix.shape[1])
        hs = sum(pix[:, np.clip(xs + i, 0, len(xs) - 1)] for i in range(-r, r + 1))
        for y in rows:
            want = sum(hs[np.clip(y + j, 0, H - 1) - need[0]] for j in range(-r, r + 1))
            assert np.array_equal(C[y], want), (y, U.describe_mismatch("C", C[y], want))
    del C
    assert np.array_equal(eng.compute_host(a, (b + 30).astype(np.uint8)), base)
    assert (base != -16).mean() > 0.3
