"""The match confidence on the CPU: the numpy restatement (tests/confidence_ref.py) against known answers, and the property
that makes the quantity worth keeping -- for integer u in 0 .. 100 upstream's uniqueness test keeps a pixel iff
conf_raw >= u -- against both oracles.  Needs no GPU."""
import os
import re

import numpy as np
import pytest

import bruteforce_color as BC
import confidence_ref as CR
import parity_util as U
from oracle import oracle as O
from oracle import volume_oracle as V
from stereo_reconstruction_cv_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U_LIST = (0, 1, 5, 10, 15, 25, 40, 70, 99, 100)


def _row(D, **at):
    """one pixel's S vector: 1000 everywhere but at the given disparities"""
    s = np.full((1, 1, D), 1000, np.int16)
    for d, v in at.items():
        s[0, 0, int(d[1:])] = v
    return s


def test_known_answers():
    c, best, minS, far = CR.conf_raw_rows(_row(16, d5=10, d9=40))
    assert (c[0, 0], best[0, 0], minS[0, 0], far[0, 0]) == (75, 5, 10, 40)           # (40 - 10) * 100 // 40
    # the neighbours of the best do not count as competitors: far stays at the 1000 of the background
    c, _, _, far = CR.conf_raw_rows(_row(16, d5=10, d4=11, d6=12))
    assert (c[0, 0], far[0, 0]) == (99, 1000)
    # far == minS -> 0; a tie on the minimum takes the FIRST d
    c, best, _, _ = CR.conf_raw_rows(_row(16, d3=10, d9=10))
    assert (c[0, 0], best[0, 0]) == (0, 3)
    # far == 0 -> 100 (minS is 0 too)
    c, _, minS, far = CR.conf_raw_rows(np.zeros((1, 1, 16), np.int16))
    assert (c[0, 0], minS[0, 0], far[0, 0]) == (100, 0, 0)
    # every cost saturated: minS = far = 32767 -> 0
    c, best, minS, far = CR.conf_raw_rows(np.full((1, 1, 16), 32767, np.int16))
    assert (c[0, 0], best[0, 0], minS[0, 0], far[0, 0]) == (0, 0, 32767, 32767)
    # best at d = 0: only d = 1 is excluded (d = 2 competes); best at d = D - 1: only d = D - 2
    c, best, _, far = CR.conf_raw_rows(_row(16, d0=10, d1=11, d2=20))
    assert (c[0, 0], best[0, 0], far[0, 0]) == (50, 0, 20)
    c, best, _, far = CR.conf_raw_rows(_row(16, d15=10, d14=11, d13=20))
    assert (c[0, 0], best[0, 0], far[0, 0]) == (50, 15, 20)
    # C division: (far - minS) * 100 / far truncates
    c, _, _, _ = CR.conf_raw_rows(_row(16, d5=1, d9=3))
    assert c[0, 0] == 66
    # the frame: 0 outside the matched columns
    m = CR.conf_raw(np.concatenate([_row(16, d5=10, d9=40)] * 3, axis=1), W=30, minX1=20)
    assert m.shape == (1, 30) and (m[:, :20] == 0).all() and (m[:, 20:23] == 75).all() and (m[:, 23:] == 0).all()


def test_the_property_is_an_identity_of_the_integers():
    """far * (100 - u) >= minS * 100  <=>  (far - minS) * 100 // far >= u   for 0 <= minS <= far <= 32767, far > 0, and
    u in 0 .. 100 (x >= u <=> floor(x) >= u for integer u) -- on a dense sample of the domain and all 101 ratios."""
    rng = np.random.default_rng(5)
    far = np.concatenate([np.arange(1, 600), rng.integers(1, 32768, 4000), [32767, 32766]]).astype(np.int64)
    for f in far[::7]:
        m = np.arange(0, f + 1, max(1, f // 997), dtype=np.int64)
        m = np.unique(np.concatenate([m, [f, max(f - 1, 0)]]))
        conf = (f - m) * 100 // f
        for u in range(101):
            assert np.array_equal(f * (100 - u) >= m * 100, conf >= u), (f, u)


# (H, W, D, minDisparity, mode, blockSize, seed): the three shapes of the issue, then one more per mode
_GRAY_CASES = [(40, 200, 64, 0, 0, 5, 11), (33, 150, 32, -3, 1, 5, 12), (30, 180, 128, 0, 1, 3, 13),
               (36, 190, 48, 4, 0, 7, 14), (28, 170, 16, 0, 1, 9, 15)]


def _check_property(compute, l, r, p, minD):
    """compute: an oracle's sgbm_compute.  disp12MaxDiff = 100000 switches the LR check off (a value <= 0 would become 1)."""
    q = dict(p, disp12MaxDiff=100000, speckleWindowSize=0, speckleRange=0)
    _, t = compute(l, r, taps=True, **dict(q, uniquenessRatio=10))
    assert t["headroom_ok"]
    S = t["S"]
    H, W = l.shape[:2]
    minX1 = W - S.shape[1] + min(minD, 0)
    c, _, minS, _ = CR.conf_raw_rows(S)
    assert CR.deciles_populated(c) >= 8, np.bincount(c.ravel() // 10, minlength=11)
    invalid = (minD - 1) * 16
    kept10 = t["disp_raw"][:, minX1:minX1 + S.shape[1]] != invalid
    assert kept10.any() and (~kept10).any()
    for u in U_LIST:
        _, tu = compute(l, r, taps=True, **dict(q, uniquenessRatio=u))
        assert np.array_equal(tu["S"], S)                      # the volume does not depend on the ratio
        valid = tu["disp_raw"][:, minX1:minX1 + S.shape[1]] != invalid
        want = (c >= u) & (minS != CR.MAX_COST)
        assert np.array_equal(valid, want), (u, int((valid != want).sum()))
        assert (tu["disp_raw"][:, :minX1] == invalid).all() and (tu["disp_raw"][:, minX1 + S.shape[1]:] == invalid).all()


@pytest.mark.parametrize("H,W,D,minD,mode,bs,seed", _GRAY_CASES)
def test_conf_raw_is_the_largest_ratio_that_keeps_the_pixel(H, W, D, minD, mode, bs, seed):
    l, r, _ = synth.make_pair(H, W, D, seed)
    _check_property(O.sgbm_compute, l, r, U.params(D, bs, minD, mode), minD)


def test_the_property_in_mode_hh4_and_on_a_colour_pair():
    l, r, _ = synth.make_pair(34, 190, 64, 21)
    _check_property(V.sgbm_compute, l, r, U.params(64, 5, 0, 3), 0)
    L3, R3 = BC.colour_pair(30, 170, 32, seed=22)
    _check_property(V.sgbm_compute, L3, R3, U.params(32, 3, 0, 0, penalty="plain"), 0)
    L3, R3 = BC.colour_pair(26, 200, 64, seed=23, minD=-2)
    _check_property(V.sgbm_compute, L3, R3, U.params(64, 5, -2, 1, penalty="plain"), -2)


@pytest.mark.parametrize("H,W,D,minD,mode,bs,seed", _GRAY_CASES[:3])
def test_final_map_masks_the_margin(H, W, D, minD, mode, bs, seed):
    """conf == conf_raw where the oracle's final map (LR check, median, speckle filter) is valid, 0 elsewhere -- and the
    filters do take pixels away that the winner-take-all kept, so the two maps differ."""
    l, r, _ = synth.make_pair(H, W, D, seed)
    p = U.params(D, bs, minD, mode, speckleWindowSize=40, speckleRange=1)
    disp, t = O.sgbm_compute(l, r, taps=True, **p)
    minX1 = W - t["S"].shape[1] + min(minD, 0)
    raw = CR.conf_raw(t["S"], W, minX1)
    conf = CR.conf_final(raw, disp, minD)
    valid = disp != (minD - 1) * 16
    assert np.array_equal(conf[valid], raw[valid]) and (conf[~valid] == 0).all()
    assert valid.any() and ((raw > 0) & ~valid).any()
    assert (raw[:, :minX1] == 0).all() and (raw[:, minX1 + t["S"].shape[1]:] == 0).all()


def test_masking_helper_matches_boolean_indexing():
    """valid_points(..., confidence, min_confidence) zeroes the disparity where the confidence is too low and then runs the
    existing compaction: the helper alone, against numpy (the compaction itself needs the GPU: tests/test_gpu_confidence.py)."""
    from stereo_reconstruction_cv_amd import mask_by_confidence
    rng = np.random.default_rng(3)
    disp = rng.uniform(-2, 60, (17, 23)).astype(np.float32)
    conf = rng.integers(0, 101, (17, 23)).astype(np.uint8)
    for u in (0, 1, 37, 100, 101):
        m = mask_by_confidence(disp, conf, u)
        assert m.dtype == disp.dtype and m is not disp
        assert np.array_equal(m > 0, (disp > 0) & (conf >= u))
        assert np.array_equal(m[conf >= u], disp[conf >= u])
    d16 = (disp * 16).astype(np.int16)
    assert np.array_equal(mask_by_confidence(d16, conf, 50) > 0, (d16 > 0) & (conf >= 50))
    import stereo_reconstruction_cv_amd as cv
    with pytest.raises(cv.error):
        mask_by_confidence(disp, conf[:-1], 3)


def test_interface_lists_the_additions():
    """header, binding and library agree on what is new; the ABI version stays"""
    txt = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    assert re.search(r"SGM_OPT_CONFIDENCE\s*=\s*10\b", txt) and re.search(r"SGM_TAP_CONF_RAW\s*=\s*4\b", txt)
    assert re.search(r"SGM_TAP_CONF\s*=\s*5\b", txt)
    assert (_lib.SGM_OPT_CONFIDENCE, _lib.SGM_TAP_CONF_RAW, _lib.SGM_TAP_CONF) == (10, 4, 5)
    extra = open(os.path.join(ROOT, "include", "sgm_hip_confidence.h")).read()
    declared = sorted(set(re.findall(r"\b(sgm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", extra, flags=re.S))))
    assert declared == sorted(_lib.CONFIDENCE_EXPORTS) == ["sgm_bind_confidence_device"]
    assert '#include "sgm_hip_confidence.h"' in txt and all(hasattr(_lib.load(), n) for n in declared)
    assert re.search(r"#define SGM_ABI_VERSION 4\b", txt)
    assert "follow-up" in txt and "sgm_compute_batch" in txt and "sgm_compute" in extra
    import stereo_reconstruction_cv_amd as cv
    assert callable(cv.StereoSGBM.computeWithConfidence)


def test_no_kernel_gained_scratch_and_the_confidence_kernels_use_none():
    """resource remarks of the build: every k_wta_conf_t instantiation and k_conf_final without scratch"""
    path = os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "resource_usage.txt")
    txt = open(path).read()
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", txt, flags=re.S)
    conf = [(n, int(s)) for n, s in blocks if "k_wta_conf_t" in n or "k_conf_final" in n]
    assert len(conf) >= 24 + 2, len(conf)
    assert all(s == 0 for _, s in conf), [c for c in conf if c[1]]
