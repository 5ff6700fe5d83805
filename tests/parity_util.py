"""Shared helpers for the GPU parity tests: run the HIP engine through the C ABI with stage taps
and compare every stage with the CPU oracle."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd.stereo import Engine

NB = dict(disp12MaxDiff=1, preFilterCap=63, uniquenessRatio=10, speckleWindowSize=100, speckleRange=32)


def params(D, bs, minD=0, mode=0, penalty="notebook", **kw):
    """Notebook penalties by default (/root/reference/main.ipynb:659-660: P1 = 8*3*bs^2, P2 = 32*3*bs^2,
    the 3-channel formula on grayscale input -- what bench.py times); penalty="plain" gives the
    single-channel 8*bs^2 / 32*bs^2 of OpenCV's documentation."""
    ch = 3 if penalty == "notebook" else 1
    p = dict(minDisparity=minD, numDisparities=D, blockSize=bs, P1=8 * ch * bs * bs, P2=32 * ch * bs * bs, mode=mode, **NB)
    p.update(kw)
    return p


def run_hip_with_taps(left, right, p, schedule=1, sweep_rows=0, debug=0, prepass_rows=0, chain_wgs=0):
    eng = Engine(p)
    if chain_wgs:
        eng.set_option(_lib.SGM_OPT_CHAIN_WGS, chain_wgs)
    if debug:
        eng.set_option(_lib.SGM_OPT_DEBUG, debug)
    if prepass_rows:
        eng.set_option(_lib.SGM_OPT_PREPASS_ROWS, prepass_rows)
    eng.set_option(_lib.SGM_OPT_KEEP_AGGR, 1)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, schedule)
    eng.set_option(_lib.SGM_OPT_SWEEP_ROWS, sweep_rows)
    H, W = left.shape[:2]        # (H, W) gray or (H, W, 3) colour
    disp = eng.compute_host(left, right)
    _, W1 = eng.geometry(W)
    out = dict(disp=disp, disp_raw=eng.tap(_lib.SGM_TAP_DISP_RAW, H, W),
               disp_median=eng.tap(_lib.SGM_TAP_DISP_MEDIAN, H, W))
    if W1 > 0:
        out["C"] = eng.tap(_lib.SGM_TAP_COST, H, W)
        out["S"] = eng.tap(_lib.SGM_TAP_AGGR, H, W)
    out["headroom"] = eng.headroom()     # the engine's own regime record (sgm_get_headroom)
    return out


def compare_stages(left, right, p, schedule=1, sweep_rows=0, prepass_rows=0, chain_wgs=0):
    """Returns (report dict stage -> mismatch count, oracle taps)."""
    d, t = O.sgbm_compute(left, right, taps=True, **p)
    t["disp"] = d
    h = run_hip_with_taps(left, right, p, schedule, sweep_rows, prepass_rows=prepass_rows, chain_wgs=chain_wgs)
    rep = {}
    for k in ("C", "S", "disp_raw", "disp_median", "disp"):
        if k in h and k in t:
            rep[k] = int((h[k] != t[k]).sum())
    t["headroom"] = dict(ok=bool(t["headroom_ok"]), max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"])
    rep["headroom"] = int(h["headroom"] != t["headroom"])
    return rep, t, h


def headroom_equal(h, t) -> bool:
    """device-side regime record == the oracle's (max C + P2 incl. the running-sum intermediate,
    max min_d L_r + P2, and the verdict)"""
    return h["headroom"] == dict(ok=bool(t["headroom_ok"]), max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"])


def describe_mismatch(k, a, b):
    if k == "headroom":
        return f"headroom record: hip {a} != oracle {b}"
    idx = np.argwhere(a != b)
    s = f"{k}: {len(idx)} mismatches of {a.size}; first {idx[:5].tolist()}"
    if len(idx):
        i = tuple(idx[0])
        s += f" hip={a[i]} oracle={b[i]}"
    return s
