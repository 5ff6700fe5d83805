"""numpy restatement of the per-pixel match confidence (include/sgm_hip.h: SGM_TAP_CONF_RAW / SGM_TAP_CONF), from a
finished aggregated volume S [H][W1][D] -- what both oracles return as taps["S"].

    best = first d that minimises S[y][x1][.]
    minS = S[y][x1][best]
    far  = min over d with |d - best| > 1 of S[y][x1][d]
    conf_raw = 100 if far == 0 else (far - minS) * 100 // far        (0 .. 100)

conf_raw is 0 outside the matched columns [minX1, minX1 + W1); conf is conf_raw where the final disparity is valid and 0
where it is (minDisparity - 1) * 16.  Test infrastructure, not product code.
"""
from __future__ import annotations

import numpy as np

MAX_COST = 32767


def conf_raw_rows(S: np.ndarray):
    """(conf_raw, best, minS, far) of the matched columns: four (H, W1) arrays from S (H, W1, D)."""
    S = np.asarray(S)
    H, W1, D = S.shape
    assert D >= 4
    conf = np.empty((H, W1), np.uint8)
    best = np.empty((H, W1), np.int32)
    minS = np.empty((H, W1), np.int32)
    far = np.empty((H, W1), np.int32)
    d = np.arange(D, dtype=np.int32)
    step = max(1, (1 << 24) // max(W1 * D, 1))      # rows per chunk: the int32 copy of a 4K D=256 volume would be 8 GB
    for y0 in range(0, H, step):
        s = S[y0:y0 + step].astype(np.int32)
        b = s.argmin(axis=2).astype(np.int32)       # numpy's argmin returns the FIRST minimum
        m = np.take_along_axis(s, b[..., None], axis=2)[..., 0]
        outside = np.abs(d[None, None, :] - b[..., None]) > 1
        f = np.where(outside, s, np.int32(1 << 30)).min(axis=2)
        c = np.where(f == 0, 100, (f - m) * 100 // np.maximum(f, 1))
        assert c.min() >= 0 and c.max() <= 100
        conf[y0:y0 + step], best[y0:y0 + step], minS[y0:y0 + step], far[y0:y0 + step] = c, b, m, f
    return conf, best, minS, far


def conf_raw(S, W: int, minX1: int) -> np.ndarray:
    """uint8 (H, W): conf_raw in the matched columns, 0 elsewhere.  S: (H, W1, D), or None when W1 <= 0."""
    if S is None or S.shape[1] <= 0:
        raise ValueError("no matched column: use np.zeros((H, W), np.uint8)")
    H, W1, _ = S.shape
    out = np.zeros((H, W), np.uint8)
    out[:, minX1:minX1 + W1] = conf_raw_rows(S)[0]
    return out


def conf_final(raw: np.ndarray, disp: np.ndarray, minDisparity: int) -> np.ndarray:
    """conf: raw where the final map is valid, 0 where it is the invalid value"""
    return np.where(np.asarray(disp) != (minDisparity - 1) * 16, raw, np.uint8(0)).astype(np.uint8)


def deciles_populated(c: np.ndarray) -> int:
    """how many of the 11 classes 0-9, 10-19, ..., 90-99, 100 hold at least one pixel"""
    return int((np.bincount(np.asarray(c).ravel() // 10, minlength=11) > 0).sum())
