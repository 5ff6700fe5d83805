"""The colour (cn = 3) restatement of tests/bruteforce_color.py anchored to the C oracle by two exact relations on small
cases (CPU only):

  linearity          the block cost C of a colour pair is the sum of the oracle's C taps of its three channel images;
  equal channels     (I, I, I) with penalties (3 P1, 3 P2) gives the oracle's map of I with (P1, P2) -- every step after C
                     is scale-invariant (uniqueness test, sub-pixel division, LR check) while nothing saturates at 32767,
                     which each case asserts from the oracle's taps (a case that breaks it is a bad case, not a skip).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bruteforce_color as BC  # noqa: E402
import bruteforce_sgbm as BF  # noqa: E402
from oracle import oracle as O  # noqa: E402
from stereo_reconstruction_cv_amd import synth  # noqa: E402

NB = dict(disp12MaxDiff=1, preFilterCap=63, uniquenessRatio=10, speckleWindowSize=20, speckleRange=2)

CASES = [  # (H, W, D, minD, bs, mode, preFilterCap)
    (10, 44, 16, 0, 3, 0, 63),
    (9, 40, 16, -3, 5, 1, 15),
    (8, 52, 32, 2, 1, 0, 111),
]


@pytest.mark.parametrize("H,W,D,minD,bs,mode,cap", CASES)
def test_colour_cost_is_the_sum_of_the_channel_costs(H, W, D, minD, bs, mode, cap):
    L, R = BC.colour_pair(H, W, D, seed=H * W + D, minD=minD)
    p = dict(minDisparity=minD, numDisparities=D, blockSize=bs, P1=4 * bs * bs, P2=20 * bs * bs, mode=mode,
             **dict(NB, preFilterCap=cap))
    want = sum(O.sgbm_compute(np.ascontiguousarray(L[..., c]), np.ascontiguousarray(R[..., c]), taps=True, **p)[1]["C"]
               .astype(np.int64) for c in range(3))
    q = BF.normalise(**p)
    pix, _, _ = BC.pixel_cost_c3(L, R, q)
    C = BF.block_cost(pix, q["r"])
    assert C.shape == want.shape
    assert np.array_equal(C, want)
    assert pix.max() <= 3 * (2 * q["ftzero"] + 63)


def _wta_reads_unsaturated(S, uniq, k=3):
    """k * S stays below 32767 wherever the winner-take-all reads it: at the best d, its two neighbours and every d
    inside the uniqueness band (S * (100 - uniq) < min * 100)"""
    Sk = S.astype(np.int64) * k
    Sw = S.astype(np.int64)
    m = Sw.min(axis=2, keepdims=True)
    band = Sw * (100 - uniq) < m * 100 + 1
    best = Sw.argmin(axis=2)
    nb = np.zeros_like(band)
    for o in (-1, 0, 1):
        idx = np.clip(best + o, 0, S.shape[2] - 1)
        np.put_along_axis(nb, idx[..., None], True, axis=2)
    return int(Sk[band | nb].max(initial=0)) < BF.MAX_COST


@pytest.mark.parametrize("H,W,D,minD,bs,mode,cap", CASES)
def test_equal_channels_with_tripled_penalties_give_the_gray_map(H, W, D, minD, bs, mode, cap):
    I, J, _ = synth.make_pair(H, W, D, seed=7 + D + bs)
    P1, P2 = 2 * bs * bs, 7 * bs * bs
    assert 0 < P1 < P2
    p = dict(minDisparity=minD, numDisparities=D, blockSize=bs, mode=mode, **dict(NB, preFilterCap=cap))
    gray, t = O.sgbm_compute(I, J, taps=True, P1=P1, P2=P2, **p)
    # the precondition: no value the winner-take-all reads saturates once tripled, and no path state leaves the regime
    assert _wta_reads_unsaturated(t["S"], NB["uniquenessRatio"])
    assert 3 * t["max_delta"] <= BF.MAX_COST and 3 * t["max_cost_plus_p2"] <= BF.MAX_COST
    I3, J3 = np.repeat(I[..., None], 3, axis=2), np.repeat(J[..., None], 3, axis=2)
    got = BC.sgbm_c3(I3, J3, P1=3 * P1, P2=3 * P2, **p)
    assert np.array_equal(got["C"], 3 * t["C"].astype(np.int64))
    assert np.array_equal(got["disp_raw"], t["disp_raw"])
    assert np.array_equal(got["disp_median"], t["disp_median"])
    assert np.array_equal(got["disp"], gray)


def test_channel_order_does_not_matter():
    L, R = BC.colour_pair(8, 40, 16, seed=5)
    kw = dict(numDisparities=16, blockSize=3, P1=24, P2=96, **NB)
    a, b = BC.sgbm_c3(L, R, **kw), BC.sgbm_c3(L[..., ::-1].copy(), R[..., ::-1].copy(), **kw)
    assert np.array_equal(a["disp"], b["disp"]) and np.array_equal(a["C"], b["C"])
