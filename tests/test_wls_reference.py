"""The edge-aware disparity filter on the CPU: the numpy restatement of include/sgm_hip_wls.h (tests/wls_ref.py) against
answers worked out by hand and against the properties that make the filter worth having, float32 against float64, the host-side
table builder, the Python surface and the interface lists.  Needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import confidence_ref as CR
import parity_util as U
import wls_ref as WR
import stereo_reconstruction_cv_amd as cv
from oracle import oracle as O
from stereo_reconstruction_cv_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUT = WR.weights(1.5)
SCENES = [(40, 120, 1), (64, 200, 2), (33, 97, 3)]


def test_a_line_of_one_element_is_the_identity():
    x = np.array([[3.5], [-7.25]], np.float32)
    (y,) = WR.solve_lines([x], np.empty((2, 0), np.float32), np.float32(4000))
    assert np.array_equal(x, y)
    r = WR.wls_filter(np.array([[160]], np.int16), np.array([[9]], np.uint8), None, -16, 8000.0, LUT)
    assert r["out"].tolist() == [[160]] and r["out_f32"].tolist() == [[10.0]] and r["v"].tolist() == [[100.0]]
    # ... and so is the pass across a 1 x n or an n x 1 image: a row alone equals its transpose as a column alone
    d = np.array([[160, 320, -16, 200, 640, 100, 90]], np.int16)
    g = np.array([[10, 12, 40, 41, 41, 200, 3]], np.uint8)
    a, b = WR.wls_filter(d, g, None, -16, 8000.0, LUT), WR.wls_filter(d.T.copy(), g.T.copy(), None, -16, 8000.0, LUT)
    assert np.array_equal(a["out"], b["out"].T) and np.array_equal(a["out_f32"], b["out_f32"].T)


def test_two_pixels_one_iteration_match_the_closed_form():
    """(x_0 (1 + k) + x_1 k) / (1 + 2 k) with k = lambda_1 * exp(-2 / 1.5), lambda_1 = 1.5 * 8000 / 3 (T = 1).  Float accuracy:
    u is about 2.4e4 (ulp 0.002) behind a dozen roundings, divided by v = 100: 1e-3 is generous."""
    d = np.array([[160, 320]], np.int16)
    g = np.array([[10, 12]], np.uint8)
    assert WR.lambdas(8000.0, 1) == [4000.0]
    k = 4000.0 * np.exp(-2 / 1.5)
    want = [(160 * (1 + k) + 320 * k) / (1 + 2 * k), (320 * (1 + k) + 160 * k) / (1 + 2 * k)]
    assert abs(want[0] - 239.9621) < 1e-4 and abs(want[1] - 240.0379) < 1e-4
    for dt, tol in ((np.float32, 1e-3), (np.float64, 1e-6)):    # (float64: the table itself is float32, 6e-8 of k)
        r = WR.wls_filter(d, g, None, -16, 8000.0, LUT, dtype=dt, T=1)
        assert np.abs(r["q"][0] - want).max() <= tol, (dt, r["q"], want)
    assert np.abs(r["v"] - 100).max() <= 1e-9           # (float64; what float32 does to v: the test of u and v below)
    assert WR.wls_filter(d, g, None, -16, 8000.0, LUT, T=1)["out"].tolist() == [[240, 240]]


def test_lambda_zero_returns_the_input_where_confidence_is_at_least_one():
    rng = np.random.default_rng(4)
    d = rng.integers(-300, 4000, (19, 37)).astype(np.int16)
    d[rng.random(d.shape) < 0.3] = -160
    conf = rng.integers(0, 101, d.shape).astype(np.uint8)
    conf[0, :5] = 0
    g = rng.integers(0, 256, d.shape + (3,)).astype(np.uint8)
    r = WR.wls_filter(d, g, conf, -160, 0.0, LUT)
    keep = (d != -160) & (conf >= 1)
    assert np.array_equal(r["out"], np.where(keep, d, -160)) and np.array_equal(r["valid"], keep)
    assert np.array_equal(r["out_f32"], np.where(keep, d / np.float32(16), 0).astype(np.float32))
    assert np.array_equal(WR.wls_filter(d, g, None, -160, 0.0, LUT)["out"], d)


def test_a_constant_map_comes_back_as_that_constant():
    """u = 400 v before the first pass and both go through the same linear operator, so u / v = 400 up to rounding: a few
    roundings of relative 6e-8 per element and pass on values near 400 -- 5e-3 is two orders above that and far below the 0.5
    that would move the rounded map."""
    rng = np.random.default_rng(8)
    for g in (rng.integers(0, 256, (31, 53)).astype(np.uint8), rng.integers(100, 104, (31, 53, 3)).astype(np.uint8)):
        d = np.full((31, 53), 400, np.int16)
        d[rng.random(d.shape) < 0.5] = -16
        conf = rng.integers(1, 101, d.shape).astype(np.uint8)
        r = WR.wls_filter(d, g, conf, -16, 8000.0, LUT)
        assert r["valid"].sum() >= (d != -16).sum()
        assert (r["out"][r["valid"]] == 400).all() and (r["out"][~r["valid"]] == -16).all()
        assert np.abs(r["q"][r["valid"]] - 400).max() <= 5e-3
    assert r["valid"].all()             # (the smooth guide carries the constant into every hole)


def test_u_and_v_are_smoothed_with_the_same_coefficients():
    """Every row of the system sums to one (b = 1 - a - c), so a constant v stays constant: all valid, no confidence map ->
    v = 100 within float noise.  The noise: the elimination forms m = b - a c' with b about 1 + 2 k and a c' about k, which
    cancels log2(k) bits, so a step is good to about k * 2^-24 relative, k <= lambda_1 = 1.5 * 8000 * 16 / 63; the bound allows
    eight such steps.  u carries the SAME error in c' and r, which is why u / v is far better than either (the constant-map
    test: 5e-3 in 400)."""
    rng = np.random.default_rng(9)
    d = rng.integers(0, 1000, (29, 61)).astype(np.int16)
    g = (rng.integers(0, 4, d.shape) * 60 + rng.integers(0, 3, d.shape)).astype(np.uint8)
    r = WR.wls_filter(d, g, None, -16, 8000.0, LUT)
    assert np.abs(r["v"] - 100).max() <= 100 * 8 * WR.lambdas(8000.0)[0] * 2.0 ** -24 and r["valid"].all()
    r64 = WR.wls_filter(d, g, None, -16, 8000.0, LUT, dtype=np.float64)
    assert np.abs(r64["v"] - 100).max() <= 1e-9


@pytest.mark.parametrize("H,W,seed", SCENES)
def test_quality_on_a_layered_scene(H, W, seed):
    """Conditions, not measurements: full density, no pixel more than one pixel (16 units) off, the mean error at most a quarter
    of the input's.  (What the reference gives: DESIGN.md 4.15.)"""
    s = WR.layered_scene(H, W, seed)
    ok = s["disp"] != s["invalid"]
    assert 0.7 < ok.mean() < 0.9
    err_in = np.abs(s["disp"].astype(np.int32) - s["truth"])[ok].mean()
    r = WR.wls_filter(s["disp"], s["guide"], s["conf"], s["invalid"], 8000.0, LUT)
    err = np.abs(r["out"].astype(np.int32) - s["truth"])
    print(f"layered {H}x{W}: input mean {err_in:.2f}, output mean {err.mean():.3f} max {err.max()}, ratio {err_in / err.mean():.1f}")
    assert r["valid"].all() and (r["out"] != s["invalid"]).all()
    assert err.max() <= 16
    assert err.mean() <= err_in / 4


def _oracle_input():
    """a computeWithConfidence-shaped input: the frozen oracle's map and confidence_ref's masked margin"""
    H, W, D = 48, 320, 64
    l, r, _ = synth.make_pair(H, W, D, 7)
    p = U.params(D, 5, 0, 1)
    disp, t = O.sgbm_compute(l, r, taps=True, **p)
    minX1 = W - t["S"].shape[1]
    conf = CR.conf_final(CR.conf_raw(t["S"], W, minX1), disp, 0)
    return dict(disp=disp, guide=l, conf=conf, invalid=-16)


def test_float32_against_float64():
    """on pixels valid in both, the quotients differ by at most a quarter of a unit (1/64 px)"""
    worst = 0.0
    for s in [WR.layered_scene(*a) for a in SCENES] + [_oracle_input()]:
        a = WR.wls_filter(s["disp"], s["guide"], s["conf"], s["invalid"], 8000.0, LUT)
        b = WR.wls_filter(s["disp"], s["guide"], s["conf"], s["invalid"], 8000.0, LUT, dtype=np.float64)
        both = a["valid"] & b["valid"]
        assert both.mean() > 0.5
        dq = float(np.abs(a["q"].astype(np.float64) - b["q"])[both].max())
        print(f"float32 vs float64 {s['disp'].shape}: max |dq| {dq:.4f}, rounded maps differ in {int((a['out'] != b['out'])[both].sum())}")
        worst = max(worst, dq)
    assert worst <= 0.25


def test_sgm_wls_weights():
    L = _lib.load()
    for sigma in (1.5, 0.5, 10.0, 300.0):
        lut = np.full(256, -1, np.float32)
        assert L.sgm_wls_weights(C.c_double(sigma), lut.ctypes.data) == 0
        want = WR.weights(sigma)
        assert lut[0] == 1.0 and (np.diff(lut) <= 0).all() and (lut >= 0).all()
        assert (np.abs(lut.astype(np.float64) - want) <= np.spacing(np.maximum(lut, want))).all(), sigma
        assert np.array_equal(cv.wls_weights(sigma), lut)
    for bad in (0.0, -1.5, float("nan"), float("inf")):
        assert L.sgm_wls_weights(C.c_double(bad), lut.ctypes.data) == -1, bad        # SGM_ERR_INVALID_ARG
        assert b"sigma" in L.sgm_last_error()
        with pytest.raises(cv.error):
            cv.wls_weights(bad)
    assert L.sgm_wls_weights(C.c_double(1.5), None) == -1


def test_python_surface():
    f = cv.createDisparityWLSFilter()
    assert isinstance(f, cv.DisparityWLSFilter) and (f.getLambda(), f.getSigmaColor()) == (8000.0, 1.5)
    assert f.defaultInvalid() == -16
    f.setLambda(125)
    f.setSigmaColor(0.75)
    assert (f.getLambda(), f.getSigmaColor()) == (125.0, 0.75)
    for bad in (-1, 1e7 + 1, float("nan")):
        with pytest.raises(cv.error, match="setLambda"):
            f.setLambda(bad)
    for bad in (0, -2, float("inf"), float("nan")):
        with pytest.raises(cv.error, match="setSigmaColor"):
            f.setSigmaColor(bad)
    assert (f.getLambda(), f.getSigmaColor()) == (125.0, 0.75)
    m = cv.StereoSGBM_create(minDisparity=-9, numDisparities=64)
    assert cv.createDisparityWLSFilter(m).defaultInvalid() == -160
    assert cv.createDisparityWLSFilter(cv.StereoSGBM_create(minDisparity=3)).defaultInvalid() == 32
    assert callable(cv.StereoSGBM.computeFiltered) and callable(cv.Engine.wls_filter_host) and callable(cv.Engine.wls_filter_device)
    # validation comes before any engine is asked for: every refusal is sgm.error, GPU or not
    d, g, c = np.zeros((6, 9), np.int16), np.zeros((6, 9), np.uint8), np.zeros((6, 9), np.uint8)
    with pytest.raises(cv.error, match="same size"):
        f.filter(d, g[:, :8])
    with pytest.raises(cv.error, match="same size"):
        f.filter(d, g, c[:5])
    with pytest.raises(cv.error, match="same size"):
        f.filter(d, np.zeros((9, 6, 3), np.uint8))
    with pytest.raises(cv.error, match="CV_16SC1"):
        f.filter(d.astype(np.int32), g)
    with pytest.raises(cv.error, match="CV_8U"):
        f.filter(d, g.astype(np.float32))
    with pytest.raises(cv.error, match="CV_8UC1"):
        f.filter(d, g, c.astype(np.int16))
    for gbad in (np.zeros((6, 9, 2), np.uint8), np.zeros((6, 9, 4), np.uint8), np.zeros((6, 9, 3, 1), np.uint8), np.zeros(54, np.uint8)):
        with pytest.raises(cv.error, match=r"\(H, W\) or \(H, W, 3\)"):
            f.filter(d, gbad)
    with pytest.raises(cv.error, match=r"\(H, W\)"):
        f.filter(np.zeros((6, 9, 1), np.int16), g)
    with pytest.raises(cv.error, match="empty"):
        f.filter(np.zeros((0, 9), np.int16), np.zeros((0, 9), np.uint8))
    with pytest.raises(cv.error, match="empty"):
        f.filter(np.zeros((6, 0), np.int16), np.zeros((6, 0, 3), np.uint8))
    with pytest.raises(cv.error, match="outside int16"):
        f.filter(d, g, invalid=40000)


def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; sgm_hip.h's own list and the ABI version stay"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "sgm_hip_wls.h")).read()
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", extra, flags=re.S))))
    assert declared == sorted(_lib.WLS_EXPORTS) == ["sgm_wls_filter", "sgm_wls_filter_device", "sgm_wls_weights"]
    assert '#include "sgm_hip_wls.h"' in txt and all(hasattr(_lib.load(), n) for n in declared)
    assert not set(_lib.WLS_EXPORTS) & set(_lib.EXPORTS)
    assert "NOT that filter bit" in extra and "createDisparityWLSFilter" in extra


def test_the_abi_version_is_still_4():
    assert _lib.load().sgm_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define SGM_ABI_VERSION 4\b", open(os.path.join(ROOT, "include", "sgm_hip.h")).read())
