"""numpy restatement of the right-view disparity map (include/sgm_hip.h: SGM_OPT_RIGHT_VIEW, SGM_TAP_RIGHT_RAW /
SGM_TAP_RIGHT), from a finished aggregated volume S [H][W1][D] -- what both oracles return as taps["S"].

With minX1, W1, D, minD as sgm_geometry gives them, INV = (minD - 1) * 16 and u = uniquenessRatio:

    matched columns   xr = minX1 - minD + xr1, xr1 in [0, W1); every other column is INV
    candidates        k in [0, n), n = min(D, W1 - xr1), with the cost SR(k) = S[y][xr1 + k][k] (a diagonal of the row)
    winner            best = first k that minimises SR, minS = SR(best); rejected if minS == 32767 or some k < n with
                      |k - best| > 1 has SR(k) * (100 - u) < minS * 100
    sub-pixel         only for 0 < best < n - 1: den = max(SR(best-1) + SR(best+1) - 2 minS, 1),
                      d1 = best * 16 + ((SR(best-1) - SR(best+1)) * 16 + den) / (2 den) + minD * 16   (C division)
    right-to-left     dL(x) = the left winner-take-all's integer disparity best + minD (before the left LR check), minD - 1
                      where it rejected the pixel or x is no matched left column.  lo = d1 >> 4, hi = (d1 + 15) >> 4,
                      xa = xr + lo, xb = xr + hi; if both lie in [0, W): kill iff dL(xa) >= minD and |dL(xa) - lo| > d12
                      and dL(xb) >= minD and |dL(xb) - hi| > d12                                  -> right_raw
    final             right = filterSpeckles(median3x3(right_raw), INV, speckleWindowSize, 16 * speckleRange)

uniquenessRatio < 0 becomes 10 and disp12MaxDiff <= 0 becomes 1, as for the left map.  Test infrastructure, not product code.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import oracle as O

MAX_COST = 32767


def _chunks(fn, H, step):
    """fn(y0) for every chunk of `step` rows; large frames on a few threads (numpy releases the lock in its loops)"""
    starts = list(range(0, H, step))
    if len(starts) < 4:
        for y0 in starts:
            fn(y0)
        return
    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(fn, starts))


def _cdiv(a, b):
    """C integer division (toward zero) of int arrays, b > 0"""
    return np.where(a >= 0, a // b, -((-a) // b))


def _wta(cost, valid, u):
    """cost (..., K) int16 (>= 0), valid (..., K) bool with valid[..., 0] set: (best, minS, keep) of the winner-take-all with
    the ratio test over the valid candidates"""
    K = cost.shape[-1]
    c = np.where(valid, cost, np.int16(MAX_COST))             # (an invalid k never wins a tie: every valid k is smaller)
    best = c.argmin(axis=-1).astype(np.int32)                 # numpy's argmin returns the FIRST minimum
    minS = np.take_along_axis(c, best[..., None], axis=-1)[..., 0].astype(np.int32)
    k = np.arange(K, dtype=np.int32)
    outside = valid & (np.abs(k - best[..., None]) > 1)
    w = 100 - u
    if w > 0:    # some outside k with SR(k) * w < minS * 100  <=>  the smallest outside SR(k) does (w > 0)
        far = np.where(outside, cost, np.int16(MAX_COST)).min(axis=-1).astype(np.int32)
        bad = outside.any(axis=-1) & (far * w < minS * 100)
    else:
        bad = (outside & (cost.astype(np.int32) * w < minS[..., None] * 100)).any(axis=-1)
    return best, minS, ~bad & (minS != MAX_COST)


def left_winners(S, u):
    """(best, keep) of the left winner-take-all over S (H, W1, D): the WTA record the engine keeps per matched left pixel"""
    S = np.asarray(S)
    H, W1, D = S.shape
    best = np.empty((H, W1), np.int32)
    keep = np.empty((H, W1), bool)
    step = max(1, (1 << 23) // max(W1 * D, 1))
    ones = np.ones((1, 1, D), bool)
    def rows(y0):
        s = S[y0:y0 + step]
        b, _, kp = _wta(s, np.broadcast_to(ones, s.shape), u)
        best[y0:y0 + step], keep[y0:y0 + step] = b, kp

    _chunks(rows, H, step)
    return best, keep


def diagonals(S):
    """(SR, valid): SR[y][xr1][k] = S[y][xr1 + k][k] for k < n = min(D, W1 - xr1), int16 (anything where not valid) -- a
    strided view of a copy of S with D columns of padding behind every row, so that no diagonal leaves its row"""
    S = np.asarray(S)
    H, W1, D = S.shape
    pad = np.empty((H, W1 + D, D), np.int16)
    pad[:, :W1] = S
    pad[:, W1:] = MAX_COST
    st = pad.strides
    SR = np.lib.stride_tricks.as_strided(pad, (H, W1, D), (st[0], st[1], st[1] + st[2]), writeable=False)
    xr1 = np.arange(W1, dtype=np.int64)[:, None]
    k = np.arange(D, dtype=np.int64)[None, :]
    return SR, np.broadcast_to((xr1 + k < W1)[None], SR.shape)


def right_raw(S, W: int, minX1: int, minD: int, uniquenessRatio: int = 10, disp12MaxDiff: int = 1) -> np.ndarray:
    """int16 (H, W): the right-view map after winner-take-all, sub-pixel step and right-to-left check"""
    S = np.asarray(S)
    H, W1, D = S.shape
    assert W1 > 0
    u = uniquenessRatio if uniquenessRatio >= 0 else 10
    d12 = disp12MaxDiff if disp12MaxDiff > 0 else 1
    INV = (minD - 1) * 16
    # the left winners as a full-width row of integer disparities
    lb, lk = left_winners(S, u)
    dL = np.full((H, W), minD - 1, np.int32)
    dL[:, minX1:minX1 + W1] = np.where(lk, lb + minD, minD - 1)
    out = np.full((H, W), INV, np.int32)
    x0 = minX1 - minD
    assert x0 >= 0 and x0 + W1 <= W
    n = np.minimum(D, W1 - np.arange(W1, dtype=np.int32))[None, :]
    step = max(1, (1 << 23) // max(W1 * D, 1))
    def rows_of(y0):
        SR, valid = diagonals(S[y0:y0 + step])
        best, minS, keep = _wta(SR, valid, u)
        sm = np.take_along_axis(SR, np.maximum(best - 1, 0)[..., None], axis=-1)[..., 0].astype(np.int32)
        sp = np.take_along_axis(SR, np.minimum(best + 1, D - 1)[..., None], axis=-1)[..., 0].astype(np.int32)
        den = np.maximum(sm + sp - 2 * minS, 1)
        frac = np.where((best > 0) & (best < n - 1), _cdiv((sm - sp) * 16 + den, 2 * den), 0)
        d1 = best * 16 + frac + minD * 16
        lo, hi = d1 >> 4, (d1 + 15) >> 4
        xr = x0 + np.arange(W1, dtype=np.int32)[None, :]
        xa, xb = xr + lo, xr + hi
        inside = (xa >= 0) & (xa < W) & (xb >= 0) & (xb < W)
        rows = np.arange(SR.shape[0])[:, None] + y0
        da = dL[rows, np.clip(xa, 0, W - 1)]
        db = dL[rows, np.clip(xb, 0, W - 1)]
        kill = inside & (da >= minD) & (np.abs(da - lo) > d12) & (db >= minD) & (np.abs(db - hi) > d12)
        out[y0:y0 + step, x0:x0 + W1] = np.where(keep & ~kill, d1, INV)

    _chunks(rows_of, H, step)
    assert out.min() >= -32768 and out.max() <= 32767
    return out.astype(np.int16)


def right_final(raw: np.ndarray, minD: int, speckleWindowSize: int = 0, speckleRange: int = 0) -> np.ndarray:
    """median3x3, then the speckle filter under upstream's condition for the left map (speckleRange >= 0, window > 0)"""
    out = O.median3x3(np.ascontiguousarray(raw))
    if speckleRange >= 0 and speckleWindowSize > 0:
        out = O.filter_speckles(out, (minD - 1) * 16, speckleWindowSize, 16 * speckleRange)
    return out


def right_view(S, W: int, minX1: int, p: dict):
    """(right_raw, right) for the parameter dict of a compute (tests/parity_util.py: params).  S: (H, W1, D)."""
    raw = right_raw(S, W, minX1, p["minDisparity"], p.get("uniquenessRatio", 10), p.get("disp12MaxDiff", 1))
    return raw, right_final(raw, p["minDisparity"], p.get("speckleWindowSize", 0), p.get("speckleRange", 0))


def all_invalid(H: int, W: int, minD: int) -> np.ndarray:
    """the right map of a frame without a matched column (W1 <= 0)"""
    return np.full((H, W), (minD - 1) * 16, np.int16)
