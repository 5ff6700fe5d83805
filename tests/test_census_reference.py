"""The census cost's definition (tests/census_ref.py, the yardstick of tests/test_gpu_census.py) against answers worked out by
hand, its invariance, a quality floor against the Birchfield-Tomasi cost, the plan readout sgm_debug_plan_cost and the Python
surface of the option.  Needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import bruteforce_sgbm as BF
import census_ref as CE
import stereo_reconstruction_cv_amd as sgm
from stereo_reconstruction_cv_amd import _lib, synth


def bits(x):
    return bin(int(x)).count("1")


# ---- the definition ------------------------------------------------------------------------------------------------------------
def test_constant_image_has_equal_descriptors_and_zero_cost():
    img = np.full((9, 40), 77, np.uint8)
    d = CE.descriptors(img)
    assert (d == d[0, 0]).all() and d[0, 0] == 0          # nothing is strictly darker than the pixel itself
    pix = CE.pixel_cost(img, img, 0, 16)
    assert pix.shape == (9, 24, 16) and not pix.any()
    assert not CE.block_cost(pix, 2).any()


def test_one_bright_pixel():
    """every one of the 62 neighbours is darker than the bright pixel, and nothing is darker than any other pixel (the
    bright one is a neighbour of some, but it is not darker): one descriptor of 62 ones, all others zero"""
    H, W, D, minD = 11, 60, 16, 0
    y0, x0, d0 = 5, 40, 6
    left = np.full((H, W), 100, np.uint8)
    right = left.copy()
    left[y0, x0] = 101
    right[y0, x0 - d0] = 200
    dl, dr = CE.descriptors(left), CE.descriptors(right)
    assert bits(dl[y0, x0]) == 62 and bits(dr[y0, x0 - d0]) == 62
    assert np.count_nonzero(dl) == 1 and np.count_nonzero(dr) == 1
    pix = CE.pixel_cost(left, right, minD, D)
    minX1, W1 = CE.geometry(W, minD, D)
    assert (minX1, W1) == (16, 44)
    want = np.zeros((H, W1, D), np.int64)
    want[y0, x0 - minX1, :] = 62                      # the bright left pixel against a flat right pixel ...
    want[y0, x0 - minX1, d0] = 0                      # ... but not against its own image
    for k in range(D):                                # a flat left pixel against the bright right pixel
        xi = x0 - d0 + k - minX1
        if 0 <= xi < W1 and k != d0:
            want[y0, xi, k] = 62
    assert np.array_equal(pix, want)
    C1 = CE.block_cost(pix, 0)
    assert np.array_equal(C1, pix)                    # blockSize 1: the plain census cost


def test_one_bright_pixel_block_sum_by_hand():
    """the 3 x 3 sum at the bright pixel's own disparity is 0: at index d0 every left pixel x of the window looks at right
    pixel x - d0, and the only descriptor pair that differs would need x = x0 on one side only"""
    H, W, D = 11, 60, 16
    y0, x0, d0 = 5, 40, 6
    left = np.full((H, W), 100, np.uint8)
    right = left.copy()
    left[y0, x0] = 101
    right[y0, x0 - d0] = 200
    C3 = CE.block_cost(CE.pixel_cost(left, right, 0, D), 1)
    xi = x0 - 16
    assert C3[y0, xi, d0] == 0
    # at index d0 + 1: left x0 (bright) against right x0 - d0 - 1 (flat): 62; left x0 + 1 (flat) against right x0 - d0
    # (bright): 62; both inside the window of (y0, x0)
    assert C3[y0, xi, d0 + 1] == 124
    assert C3[y0, xi, d0 - 1] == 124                  # mirror image: left x0 - 1 against right x0 - d0
    assert C3[y0, xi, 0] == 62                        # far from d0 only the bright left pixel itself differs


def _dark_columns(t):
    """columns among dx = -4..-1 that lie left of a step edge t columns to the left of the pixel (t < 0: the pixel is on
    the dark side)"""
    return 0 if t < 0 else max(4 - t, 0)


def test_vertical_step_edge():
    """dark | bright: a bright pixel t columns right of the edge has 4 - t dark columns of 7 neighbours each, the dark
    sets are nested, so the Hamming distance of two pixels is 7 * |difference of their dark-column counts|"""
    H, W, D, minD, xe, s = 9, 70, 16, -2, 40, 5
    left = np.full((H, W), 50, np.uint8)
    left[:, xe:] = 100
    right = np.full((H, W), 50, np.uint8)
    right[:, xe - s:] = 100                           # the same edge at disparity s
    d = CE.descriptors(left)
    for x in range(W):
        assert bits(d[4, x]) == 7 * _dark_columns(x - xe), x
    assert [bits(v) for v in d[0, xe - 1:xe + 5]] == [0, 28, 21, 14, 7, 0]
    minX1, W1 = CE.geometry(W, minD, D)
    pix = CE.pixel_cost(left, right, minD, D)
    want = np.zeros((W1, D), np.int64)
    for xi in range(W1):
        for k in range(D):
            x = xi + minX1
            want[xi, k] = 7 * abs(_dark_columns(x - xe) - _dark_columns(x - (minD + k) - (xe - s)))
    for y in range(H):
        assert np.array_equal(pix[y], want), y
    assert not pix[:, :, s - minD].any()              # the true disparity costs nothing anywhere
    # the first bright column (4 dark columns): one disparity more looks at the dark side (0), one less one column past the edge (3)
    assert pix[:, xe - minX1, s - minD + 1].tolist() == [28] * H
    assert pix[:, xe - minX1, s - minD - 1].tolist() == [7] * H


def test_border_clamping_at_the_four_corners():
    """5 x 6, values 0..29 in row-major order: what is darker than a corner once the window is clamped"""
    img = np.arange(30, dtype=np.uint8).reshape(5, 6)
    d = CE.descriptors(img)
    assert bits(d[0, 0]) == 0                         # the smallest value
    # (0, 5) = 5: darker are (0, 0..4) -- rows dy <= 0 (4 offsets, all clamped to row 0) x columns dx < 0 (4 offsets)
    assert bits(d[0, 5]) == 16
    # (4, 0) = 24: darker are rows 0..3 -- dy < 0 (3 offsets) x all 9 dx; row 4 holds itself (dx <= 0, clamped) and brighter ones
    assert bits(d[4, 0]) == 27
    # (4, 5) = 29, the largest: all darker except the 4 x 5 - 1 offsets with dy >= 0, dx >= 0 that clamp onto itself
    assert bits(d[4, 5]) == 62 - 19


def test_fast_popcount_against_a_naive_count():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 1 << 62, size=(7, 33), dtype=np.uint64)
    x[0, 0], x[0, 1] = 0, (1 << 62) - 1
    got = CE.popcount(x)
    assert got.shape == x.shape
    assert got.tolist() == [[bits(v) for v in row] for row in x]


# ---- invariance ----------------------------------------------------------------------------------------------------------------
def test_block_cost_is_invariant_under_increasing_intensity_maps():
    H, W, D = 24, 160, 32
    a, b, _ = synth.make_pair(H, W, D, 31)
    a, b = np.minimum(a, 225), np.minimum(b, 225)
    assert a.max() <= 225 and b.max() <= 225
    f = lambda v: (v + 30).astype(np.uint8)
    g = lambda v: (v + 30 * (v >= 128)).astype(np.uint8)
    assert (np.diff(f(np.arange(226)).astype(int)) > 0).all() and (np.diff(g(np.arange(226)).astype(int)) > 0).all()
    C0 = CE.block_cost(CE.pixel_cost(a, b, 0, D), 2)
    assert C0.any()
    for m in (f, g):
        assert np.array_equal(CE.block_cost(CE.pixel_cost(a, m(b), 0, D), 2), C0)
        assert np.array_equal(CE.block_cost(CE.pixel_cost(m(a), b, 0, D), 2), C0)
    q = BF.normalise(numDisparities=D, blockSize=5)
    bt0 = BF.block_cost(BF.pixel_cost(a, b, q)[0], 2)
    assert not np.array_equal(BF.block_cost(BF.pixel_cost(a, f(b), q)[0], 2), bt0)    # Birchfield-Tomasi is not


# ---- quality floor -------------------------------------------------------------------------------------------------------------
def test_quality_floor_with_and_without_an_exposure_change():
    H, W, D = 48, 320, 64
    a, b, gt = synth.make_pair(H, W, D, 7)
    p = dict(numDisparities=D, blockSize=5, P1=8 * 25, P2=32 * 25, disp12MaxDiff=1, uniquenessRatio=10, mode=1)
    b2 = (b // 2 + 10).astype(np.uint8)
    s_plain = CE.score(CE.census_sgbm(a, b, **p)["disp"], gt, D)
    s_dark = CE.score(CE.census_sgbm(a, b2, **p)["disp"], gt, D)
    s_bt = CE.score(BF.sgbm(a, b2, preFilterCap=63, **p)["disp"], gt, D)
    print(f"census {s_plain:.3f}, census on the darkened pair {s_dark:.3f}, BT on the darkened pair {s_bt:.3f}")
    assert s_plain >= 0.70 and s_dark >= 0.70
    assert s_bt < s_dark


# ---- the plan readout ----------------------------------------------------------------------------------------------------------
def _plan(p, H, W, cost, channels=1, debug=0, schedule=1):
    out = _lib.SgmDebugPlan()
    rc = _lib.load().sgm_debug_plan_cost(C.byref(_lib.SgmParams(**p)), H, W, channels, schedule, 0, 0, debug, 1, 0, 0, cost, C.byref(out))
    return rc, {n: getattr(out, n) for n, _ in _lib.SgmDebugPlan._fields_}


def _p(D, bs, **kw):
    return dict(dict(minDisparity=0, numDisparities=D, blockSize=bs, P1=8 * bs * bs, P2=32 * bs * bs, disp12MaxDiff=1, preFilterCap=63,
                     uniquenessRatio=10, speckleWindowSize=0, speckleRange=0, mode=1), **kw)


def test_plan_readout_says_which_box_route_the_census_bytes_take():
    assert _plan(_p(128, 5), 40, 500, 1) == (0, _lib.debug_plan(_p(128, 5), 40, 500, cost=1))
    assert _plan(_p(128, 5), 40, 500, 1)[1]["byte_cost"] == 1
    assert _plan(_p(128, 5, preFilterCap=200), 40, 500, 1)[1]["byte_cost"] == 1      # 62 fits a byte whatever the cap
    assert _plan(_p(128, 5, preFilterCap=200), 40, 500, 0)[1]["byte_cost"] == 0      # ... Birchfield-Tomasi's does not
    assert _plan(_p(128, 1), 40, 500, 1)[1]["byte_cost"] == 0
    assert _plan(_p(128, 13), 40, 500, 1)[1]["byte_cost"] == 0
    assert _plan(_p(128, 11), 40, 500, 1)[1]["byte_cost"] == 1
    assert _plan(_p(528, 5), 9, 800, 1)[1]["byte_cost"] == 0
    assert _plan(_p(128, 5), 40, 500, 1, debug=256)[1]["byte_cost"] == 0
    assert _plan(_p(512, 5), 2160, 3840, 1)[1]["byte_cost"] == 0                     # a byte volume of 2 GiB and more
    assert _plan(_p(256, 5), 2160, 3840, 1)[1]["byte_cost"] == 1


@pytest.mark.parametrize("H,W,D,bs,mode,sched,debug,cap", [(40, 500, 128, 5, 1, 1, 0, 63), (2160, 3840, 256, 7, 1, 2, 0, 63),
                                                            (33, 300, 32, 3, 0, 1, 4, 63), (9, 800, 528, 5, 0, 2, 256, 200),
                                                            (40, 300, 64, 13, 3, 0, 0, 0)])
def test_plan_readout_with_the_default_cost_is_the_older_readout(H, W, D, bs, mode, sched, debug, cap):
    p = _p(D, bs, mode=mode, preFilterCap=cap)
    rc, got = _plan(p, H, W, 0, debug=debug, schedule=sched)
    assert rc == 0
    assert got == _lib.debug_plan(p, H, W, schedule=sched, debug=debug)
    for conf, right in ((1, 0), (0, 1)):
        out = _lib.SgmDebugPlan()
        assert _lib.load().sgm_debug_plan_cost(C.byref(_lib.SgmParams(**p)), H, W, 1, sched, 0, 0, debug, 1, conf, right, 0, C.byref(out)) == 0
        assert {n: getattr(out, n) for n, _ in _lib.SgmDebugPlan._fields_} == _lib.debug_plan(p, H, W, schedule=sched, debug=debug,
                                                                                             confidence=conf, right_view=right)


def test_plan_readout_refuses_a_colour_census_and_unknown_costs():
    rc, _ = _plan(_p(128, 5), 40, 500, 1, channels=3)
    assert rc == -4 and "SGM_COST_CENSUS" in _lib.last_error()                        # SGM_ERR_UNSUPPORTED
    assert _plan(_p(128, 5), 40, 500, 0, channels=3)[0] == 0
    rc, _ = _plan(_p(128, 5), 40, 500, 2)
    assert rc == -1 and "SGM_OPT_COST" in _lib.last_error()                           # SGM_ERR_INVALID_ARG


# ---- the Python surface --------------------------------------------------------------------------------------------------------
def test_constants_setter_getter_and_keyword():
    assert (sgm.STEREO_COST_BT, sgm.STEREO_COST_CENSUS) == (0, 1) == (_lib.SGM_COST_BT, _lib.SGM_COST_CENSUS)
    assert _lib.SGM_OPT_COST == 12
    m = sgm.StereoSGBM_create(numDisparities=32, blockSize=5)
    assert m.getCostFunction() == sgm.STEREO_COST_BT
    m.setCostFunction(sgm.STEREO_COST_CENSUS)
    assert m.getCostFunction() == sgm.STEREO_COST_CENSUS
    m.setCostFunction(sgm.STEREO_COST_BT)
    assert m.getCostFunction() == sgm.STEREO_COST_BT
    for bad in (2, -1, "census", None, 1.0):
        with pytest.raises(sgm.error, match="setCostFunction"):
            m.setCostFunction(bad)
    assert m.getCostFunction() == sgm.STEREO_COST_BT
    m2 = sgm.StereoSGBM_create(0, 32, 5, costFunction=sgm.STEREO_COST_CENSUS)
    assert m2.getCostFunction() == sgm.STEREO_COST_CENSUS and m2.getNumDisparities() == 32 and m2.getBlockSize() == 5
    with pytest.raises(sgm.error):
        sgm.StereoSGBM_create(numDisparities=32, costFunction=7)
    # the cost function is no StereoSGBM parameter: the engine cache is keyed by the parameters alone
    assert "costFunction" not in m2._p


def test_colour_input_with_census_raises_before_any_gpu_work():
    m = sgm.StereoSGBM_create(numDisparities=16, blockSize=3, costFunction=sgm.STEREO_COST_CENSUS)
    img = np.zeros((8, 40, 3), np.uint8)
    sgm.clear_engine_cache()
    with pytest.raises(sgm.error, match="single-channel"):
        m.compute(img, img)
    with pytest.raises(sgm.error, match="single-channel"):
        m.computeWithConfidence(img, img)
    with pytest.raises(sgm.error, match="single-channel"):
        m.computeLeftRight(img, img)
    from stereo_reconstruction_cv_amd import stereo
    assert not stereo._engine_cache                    # no engine was created, let alone used
