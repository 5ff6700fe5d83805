"""Split winner-take-all on the GPU (throughput mode, MODE_HH): the chained second sweep reduces the S it holds to a raw
record per pixel (k_sweep_chain<.., SWEEP_REDUCE>) and k_wta_select decides, instead of S written once more and read back by
k_wta_t.  Same arithmetic (upstream's selection loop: SURVEY.md A.6), so for every case the
raw disparity map, the final map and the headroom record must equal the oracle's AND those of the same engine with debug
2048 (the separate pass) in every pixel.  The cases that must not take the split form are asserted to take the old path."""
import os
import subprocess
import sys

import numpy as np
import pytest

import parity_util as U
from oracle import oracle as O
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu

SEP = 2048   # csrc/sgm_debug.h: SGM_DBG_WTA_SEPARATE
_ORACLE = {}


def _params(D, mode=1, **kw):
    return U.params(D, 5, 0, mode, speckleWindowSize=30, speckleRange=2, **kw)


def _want(key, l, r, p):
    """the oracle's maps and headroom record of a pair, computed once per session"""
    if key not in _ORACLE:
        d, t = O.sgbm_compute(l, r, taps=True, **p)
        _ORACLE[key] = dict(disp=d, disp_raw=t["disp_raw"],
                            headroom=dict(ok=bool(t["headroom_ok"]), max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"]))
    return _ORACLE[key]


def _run(l, r, p, debug=0, opts=()):
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, 2)
    eng.set_option(_lib.SGM_OPT_DEBUG, debug)
    for o, v in opts:
        eng.set_option(o, v)
    H, W = l.shape
    disp = eng.compute_host(l, r)
    out = dict(disp=disp, disp_raw=eng.tap(_lib.SGM_TAP_DISP_RAW, H, W), headroom=eng.headroom())
    out["raw_bytes"] = int(_lib.load().sgm_debug_wta_raw_bytes(eng._h))
    return out


def _assert_same(got, want, what):
    for k in ("disp_raw", "disp"):
        n = int((got[k] != want[k]).sum())
        assert n == 0, f"{what}: " + U.describe_mismatch(k, got[k], np.asarray(want[k]))
    assert got["headroom"] == want["headroom"], (what, got["headroom"], want["headroom"])


def _check_split(key, l, r, p, chained=True):
    """chained: the frame has more than one band, so throughput mode chains its sweeps and the split form applies"""
    H, W = l.shape
    assert _lib.debug_wta_split(p, H, W) == chained and not _lib.debug_wta_split(p, H, W, debug=SEP)
    want = _want(key, l, r, p)
    split, sep = _run(l, r, p), _run(l, r, p, SEP)
    assert split["raw_bytes"] == (H * W * 16 if chained else 0) and sep["raw_bytes"] == 0
    _assert_same(split, want, "split form against the oracle")
    _assert_same(sep, want, "debug 2048 against the oracle")
    _assert_same(split, sep, "split form against debug 2048")
    return want


# the pinned shape (W1 = 44, bands of 12 + 12 + 12 + 4 rows); W1 = 19: a guarded tail block with an odd pixel count against
# PPS = 2; NP = 1 with PPS = 4 and W1 = 70 = 4 * 17 + 2; one row and two columns (a single band: nothing to chain, the
# plain sweep and k_wta_t run whatever the debug mask says)
@pytest.mark.parametrize("H,W,D", [(40, 300, 256), (25, 275, 256), (13, 198, 128), (1, 258, 256)])
def test_split_form_equals_oracle_and_separate_pass(H, W, D):
    l, r, _ = synth.make_pair(H, W, D, 5100 + H)
    want = _check_split(("shape", H, W, D), l, r, _params(D), chained=H > 1)
    if H > 1:
        assert (np.asarray(want["disp"])[:, D:] >= 0).mean() > 0.05, "degenerate case"      # (of the columns that can be matched)


@pytest.mark.parametrize("ratio", [0, 1, 10, 50, 99])
def test_every_positive_uniqueness_weight(ratio):
    H, W, D = 40, 300, 256
    l, r, _ = synth.make_pair(H, W, D, 5100 + H)
    _check_split(("ratio", ratio), l, r, _params(D, uniquenessRatio=ratio))


@pytest.mark.parametrize("kind", ["constant", "shift0", "shift_last"])
def test_ties_and_best_at_either_end(kind):
    """a constant pair: every cost equal, the first d wins everywhere; right = left shifted by 0 / D - 1 columns: the best
    disparity is the first / the last one, whose missing neighbour the record clamps"""
    H, W, D = 20, 300, 256
    l, _, _ = synth.make_pair(H, W, D, 77)
    if kind == "constant":
        l = np.full((H, W), 90, np.uint8)
        r = l.copy()
    else:
        s = 0 if kind == "shift0" else D - 1
        r = np.zeros_like(l)
        r[:, :W - s] = l[:, s:]
    want = _check_split(("edge", kind), l, r, _params(D))
    raw = np.asarray(want["disp_raw"])[:, D:]
    if kind == "shift0":
        assert (raw == 0).mean() > 0.25
    if kind == "shift_last":
        assert (raw == (D - 1) * 16).mean() > 0.25


@pytest.mark.parametrize("N", [3, 2])
def test_batch_shares_one_reducing_sweep(N):
    """N different pairs through one group: final maps of every pair and the headroom record.  SGM_TAP_DISP_RAW reads the
    caller's engine only, which computes pair 0 of a group; the raw maps of the other pairs live in internal engines that
    no entry point reaches, so pair 0's raw map is the one compared."""
    import torch
    H, W, D = 30, 300, 256
    p = _params(D)
    pairs = [synth.make_pair(H, W, D, 5200 + i)[:2] for i in range(3)][:N]
    dev = torch.device("cuda", 0)
    dl = [torch.from_numpy(a).to(dev) for a, _ in pairs]
    dr = [torch.from_numpy(b).to(dev) for _, b in pairs]
    ptr = lambda ts: [t.data_ptr() for t in ts]
    res = {}
    for dbg in (0, SEP):
        dd = [torch.full((H, W), -7, dtype=torch.int16, device=dev) for _ in range(N)]
        torch.cuda.synchronize()
        eng = Engine(p)
        eng.set_option(_lib.SGM_OPT_SCHEDULE, 2)
        eng.set_option(_lib.SGM_OPT_DEBUG, dbg)
        eng.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, None, ptr(dd))
        eng.synchronize()
        res[dbg] = ([t.cpu().numpy() for t in dd], eng.headroom(), int(_lib.load().sgm_debug_wta_raw_bytes(eng._h)),
                    eng.tap(_lib.SGM_TAP_DISP_RAW, H, W))
    assert res[0][2] == N * H * W * 16 and res[SEP][2] == 0       # every engine of the group holds its own raw records
    wants = [_want(("batch", i), a, b, p) for i, (a, b) in enumerate(pairs)]
    for dbg in (0, SEP):
        raw0 = res[dbg][3]
        assert np.array_equal(raw0, wants[0]["disp_raw"]), (dbg, "raw map of pair 0", int((raw0 != wants[0]["disp_raw"]).sum()))
    for i in range(N):
        for dbg in (0, SEP):
            got = res[dbg][0][i]
            assert np.array_equal(got, wants[i]["disp"]), (dbg, i, int((got != wants[i]["disp"]).sum()))
    whr = dict(ok=all(w["headroom"]["ok"] for w in wants), max_cost_plus_p2=max(w["headroom"]["max_cost_plus_p2"] for w in wants),
               max_delta=max(w["headroom"]["max_delta"] for w in wants))
    assert res[0][1] == whr and res[SEP][1] == whr


FALLBACKS = {
    "ratio100": (256, dict(uniquenessRatio=100), 1, ()),
    "partial_d192": (192, {}, 1, ()),
    "keep_aggr": (256, {}, 1, ((_lib.SGM_OPT_KEEP_AGGR, 1),)),
    "confidence": (256, {}, 1, ((_lib.SGM_OPT_CONFIDENCE, 1),)),
    "right_view": (256, {}, 1, ((_lib.SGM_OPT_RIGHT_VIEW, 1),)),
    "mode_hh4": (256, {}, 3, ()),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_fallbacks_take_the_old_path(name):
    D, kw, mode, opts = FALLBACKS[name]
    H, W = 26, D + 40
    p = _params(D, mode, **kw)
    l, r, _ = synth.make_pair(H, W, D, 5300)
    o = dict(opts)
    assert not _lib.debug_wta_split(p, H, W, keep_aggr=o.get(_lib.SGM_OPT_KEEP_AGGR, 0), confidence=o.get(_lib.SGM_OPT_CONFIDENCE, 0),
                                    right_view=o.get(_lib.SGM_OPT_RIGHT_VIEW, 0))
    a, b = _run(l, r, p, 0, opts), _run(l, r, p, SEP, opts)
    assert a["raw_bytes"] == 0 and b["raw_bytes"] == 0
    _assert_same(a, b, "default against debug 2048")
    if mode == 1:       # (MODE_HH4 has a numpy restatement of its own: tests/test_gpu_hh4.py)
        _assert_same(a, _want(("fallback", name), l, r, p), "against the oracle")


def test_engine_with_a_history_and_poisoned_buffers():
    """an engine that ran another shape (and the separate pass) before, every buffer then filled with a hostile byte: the
    raw records and the maps behind them depend on nothing the engine held.  A child process, as tests/test_gpu_history.py
    runs its walks: poison in a buffer of indices must not end the test session."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wta_split_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "WTA_SPLIT_HISTORY_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
