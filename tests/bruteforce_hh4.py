"""MODE_HH4 restated from the stage functions of tests/bruteforce_sgbm.py: the MODE_HH pipeline over the path set
{(1,0), (-1,0), (0,1), (0,-1)} -- pre-filter, pixel cost, box sum, the recurrence of SURVEY.md A.5 once per direction,
the sum clipped at 32767, then selection, median and speckle filter unchanged.  The C oracle is frozen and refuses
mode 3, so this composition is the yardstick of the HH4 tests; tests/test_hh4_reference.py ties it to known answers and
to the oracle's cost stage.  (Parity is against this restatement, not against the cv2 wheel: SURVEY.md 8c.)"""
from __future__ import annotations

import numpy as np

import bruteforce_sgbm as BF

DIRS4 = [(1, 0), (-1, 0), (0, 1), (0, -1)]


def sgbm_hh4(left, right, C=None, pixel_cost=None, select=True, **kw):
    """Returns dict(C, S, max_delta[, disp_raw, disp_median, disp]).  `C`: a block cost to aggregate instead of the
    helper's own (the oracle's tap); `pixel_cost`: the pixel-cost stage (default BF.pixel_cost; colour pairs pass
    bruteforce_color.pixel_cost_c3).  max_delta = P2 + max over pixels and the four directions of min_d L_r(p, d): the
    second word of the engine's headroom record."""
    kw = dict(kw, mode=3)
    q = BF.normalise(**kw)
    W = left.shape[1]
    pix, minX1, W1 = (pixel_cost or BF.pixel_cost)(left, right, q)
    if C is None:
        C = BF.block_cost(pix, q["r"])
    C = np.asarray(C, np.int64)
    S = np.zeros_like(C)
    mmax = 0
    for rx, ry in DIRS4:
        L = BF.aggregate_path(C, rx, ry, q["P1"], q["P2"])
        if L.size:
            mmax = max(mmax, int(L.min(axis=2).max()))
        S += L
    S = np.minimum(S, BF.MAX_COST)
    out = dict(C=C, S=S, max_delta=q["P2"] + mmax, minX1=minX1, W1=W1)
    if select:
        raw = BF.select_disparity(S, W, minX1, q)
        med = BF.median3(raw)
        out.update(disp_raw=raw, disp_median=med, disp=BF.speckle_stage(med, q))
    return out
