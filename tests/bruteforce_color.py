"""Colour (8-bit, 3-channel) restatement of upstream's calcPixelCostBT with cn = 3, built only from the
stage functions of tests/bruteforce_sgbm.py: the pixel cost of a colour pair is the sum of the three single-channel pixel
costs of its channel images; everything downstream of it is the single-channel pipeline unchanged."""
from __future__ import annotations

import numpy as np

import bruteforce_sgbm as BF


def pixel_cost_c3(left, right, q):
    pix, minX1, W1 = BF.pixel_cost(left[..., 0], right[..., 0], q)
    for c in (1, 2):
        pix = pix + BF.pixel_cost(left[..., c], right[..., c], q)[0]
    return pix, minX1, W1


def sgbm_c3(left, right, **kw):
    """Returns dict(C, S, disp_raw, disp_median, disp) for a (H, W, 3) uint8 pair."""
    assert left.ndim == 3 and left.shape[2] == 3 and left.shape == right.shape
    q = BF.normalise(**kw)
    H, W = left.shape[:2]
    pix, minX1, W1 = pixel_cost_c3(left, right, q)
    C = BF.block_cost(pix, q["r"])
    dirs = BF.DIRS8 if q["mode"] == 1 else BF.DIRS5
    S = np.zeros_like(C)
    for rx, ry in dirs:
        S += BF.aggregate_path(C, rx, ry, q["P1"], q["P2"])
    S = np.minimum(S, BF.MAX_COST)
    raw = BF.select_disparity(S, W, minX1, q)
    med = BF.median3(raw)
    return dict(C=C, S=S, disp_raw=raw, disp_median=med, disp=BF.speckle_stage(med, q))


def colour_pair(H, W, D, seed, minD=0):
    """A textured colour pair with a known shift: three differently scrambled copies of a synthetic texture, the right
    view shifted by a smooth disparity field (in [minD, minD + D))."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H, W + D + abs(minD) + 8, 3)).astype(np.float64)
    k = np.ones(3) / 3.0
    for ax in (0, 1):
        base = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, base)
    base = np.clip(base * 1.6 - 80, 0, 255)
    L = base[:, :W].astype(np.uint8)
    disp = (minD + (D // 3) + (np.arange(W) * (D // 3)) // max(W, 1)).astype(np.int64)
    R = np.empty_like(L)
    for x in range(W):
        xr = min(max(x + disp[x], 0), base.shape[1] - 1)
        R[:, x] = base[:, xr].astype(np.uint8)
    return np.ascontiguousarray(L), np.ascontiguousarray(R)
