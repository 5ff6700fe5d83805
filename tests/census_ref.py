"""The census matching cost (SGM_OPT_COST = SGM_COST_CENSUS, include/sgm_hip.h) restated in numpy, and the whole matcher
composed from it and the stage functions of tests/bruteforce_sgbm.py: the yardstick of tests/test_gpu_census.py.

    descriptor  c(y, x): one bit per offset dy in -3..3, dx in -4..4 without the centre, 1 iff
                I[clamp(y + dy)][clamp(x + dx)] < I[y][x]
    pixel cost  pix[y][xi][k] = popcount(cL[y][xi + minX1] ^ cR[y][xi + minX1 - (minD + k)])
    block cost  C = bruteforce_sgbm.block_cost(pix, blockSize // 2)

Everything behind C is bruteforce_sgbm's (bruteforce_hh4's path set for mode 3).  tests/test_census_reference.py ties the
definition to answers worked out by hand."""
from __future__ import annotations

import numpy as np

import bruteforce_hh4 as B4
import bruteforce_sgbm as BF

OFFSETS = [(dy, dx) for dy in range(-3, 4) for dx in range(-4, 5) if (dy, dx) != (0, 0)]
assert len(OFFSETS) == 62
_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.uint8)


def descriptors(img) -> np.ndarray:
    """uint64 (H, W): bit i belongs to OFFSETS[i] (the order is this file's own: only Hamming distances are observable)"""
    I = np.asarray(img)
    assert I.ndim == 2 and I.dtype == np.uint8
    H, W = I.shape
    P = np.pad(I, ((3, 3), (4, 4)), mode="edge")
    out = np.zeros((H, W), np.uint64)
    for i, (dy, dx) in enumerate(OFFSETS):
        out |= (P[3 + dy:3 + dy + H, 4 + dx:4 + dx + W] < I).astype(np.uint64) << np.uint64(i)
    return out


def popcount(x) -> np.ndarray:
    """bits set in every element of a uint64 array, through a table on its 16-bit quarters"""
    x = np.ascontiguousarray(x, np.uint64)
    return _POP16[x.view(np.uint16).reshape(x.shape + (4,))].sum(axis=-1, dtype=np.int64)


def geometry(W: int, minD: int, D: int):
    minX1 = max(minD + D, 0)
    return minX1, W + min(minD, 0) - minX1


def pixel_cost(left, right, minD: int, D: int, rows=None) -> np.ndarray:
    """pix (len(rows), W1, D) int64 for the image rows `rows` (default: all of them, in order)"""
    H, W = np.asarray(left).shape
    minX1, W1 = geometry(W, minD, D)
    if rows is None:
        rows = np.arange(H)
        cl, cr = descriptors(left), descriptors(right)
    else:
        # descriptors of the slab around the rows only: clamped row indices are what the edge padding would give
        rows = np.asarray(rows)
        lo, hi = int(rows.min()), int(rows.max())
        slab = np.clip(np.arange(lo - 3, hi + 4), 0, H - 1)
        cl, cr = (descriptors(np.asarray(im)[slab])[3:-3][rows - lo] for im in (left, right))
    pix = np.zeros((len(rows), max(W1, 0), D), np.int64)
    if W1 <= 0:
        return pix
    xs = np.arange(minX1, minX1 + W1)
    for k in range(D):
        pix[:, :, k] = popcount(cl[:, xs] ^ cr[:, xs - (minD + k)])
    return pix


def block_cost(pix, r: int) -> np.ndarray:
    return BF.block_cost(pix, r)


def max_cost(pix, C, r: int) -> int:
    """the largest value an int16 lane of upstream's cost stage would hold, without P2: max of C and of the running-sum
    intermediate C(y - 1) + hsum(min(y + r, H - 1)) (the first word of the headroom record is P2 + this)"""
    H, W1, D = pix.shape
    if C.size == 0:
        return 0
    xs = np.arange(W1)
    hs = np.zeros_like(pix)
    for i in range(-r, r + 1):
        hs += pix[:, np.clip(xs + i, 0, W1 - 1)]
    mx = int(C.max())
    for y in range(1, H):
        mx = max(mx, int((C[y - 1] + hs[min(y + r, H - 1)]).max()))
    return mx


def census_sgbm(left, right, select=True, **kw):
    """dict(C, S, disp_raw, disp_median, disp, max_cost_plus_p2, max_delta, headroom, minX1, W1) of the census matcher for
    the keyword arguments of StereoSGBM_create, modes 0, 1 and 3.  headroom: the dict Engine.headroom() returns."""
    q = BF.normalise(**kw)
    H, W = left.shape
    minX1, W1 = geometry(W, q["minD"], q["D"])
    inv = (q["minD"] - 1) * 16
    if W1 <= 0:
        raw = np.full((H, W), inv, np.int64)
        med = BF.median3(raw)
        return dict(disp_raw=raw, disp_median=med, disp=BF.speckle_stage(med, q), max_cost_plus_p2=0, max_delta=0,
                    headroom=dict(ok=True, max_cost_plus_p2=0, max_delta=0), minX1=minX1, W1=W1)
    pix = pixel_cost(left, right, q["minD"], q["D"])
    C = block_cost(pix, q["r"])
    dirs = {0: BF.DIRS5, 1: BF.DIRS8, 3: B4.DIRS4}[q["mode"]]
    S = np.zeros_like(C)
    mmax = 0
    for rx, ry in dirs:
        L = BF.aggregate_path(C, rx, ry, q["P1"], q["P2"])
        mmax = max(mmax, int(L.min(axis=2).max()))
        S += L
    S = np.minimum(S, BF.MAX_COST)
    w0, w1 = q["P2"] + max_cost(pix, C, q["r"]), q["P2"] + mmax
    out = dict(C=C, S=S, max_cost_plus_p2=w0, max_delta=w1, minX1=minX1, W1=W1,
               headroom=dict(ok=w0 <= BF.MAX_COST and w1 <= BF.MAX_COST, max_cost_plus_p2=w0, max_delta=w1))
    if select:
        raw = BF.select_disparity(S, W, minX1, q)
        med = BF.median3(raw)
        out.update(disp_raw=raw, disp_median=med, disp=BF.speckle_stage(med, q))
    return out


def score(disp16, gt, minX1: int, minD: int = 0) -> float:
    """share of the matched-column pixels whose disparity is valid and within one pixel of the ground truth"""
    d = np.asarray(disp16)[:, minX1:].astype(np.float64) / 16.0
    g = np.asarray(gt)[:, minX1:].astype(np.float64)
    ok = (np.asarray(disp16)[:, minX1:] != (minD - 1) * 16) & (np.abs(d - g) <= 1.0)
    return float(ok.mean())
