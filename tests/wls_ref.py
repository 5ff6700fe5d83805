"""The edge-aware disparity filter (include/sgm_hip_wls.h) restated in numpy: the yardstick of tests/test_wls_reference.py and
tests/test_gpu_wls.py.  dtype = np.float32 is the definition -- every operation below is one ufunc on float32 arrays, so each
is rounded on its own, in the order the header writes them; dtype = np.float64 is the same procedure in double, for comparison.
Vectorised across the lines of a pass, with a Python loop along the line."""
from __future__ import annotations

import numpy as np

T_DEFAULT = 3


def weights(sigma: float) -> np.ndarray:
    """the default table: float(exp(-k / sigma)), the exp in double"""
    return np.exp(-np.arange(256, dtype=np.float64) / float(sigma)).astype(np.float32)


def lambdas(lam: float, T: int = T_DEFAULT):
    """lambda_t for t = 1 .. T, in double (the caller rounds to its dtype)"""
    return [1.5 * float(lam) * 4.0 ** (T - t) / (4.0 ** T - 1) for t in range(1, T + 1)]


def edge_index(guide: np.ndarray, axis: int) -> np.ndarray:
    """|g_i - g_{i+1}| along axis (0: down a column, 1: along a row); 3 channels: the largest of the three"""
    g = guide.astype(np.int32)
    d = np.abs(np.diff(g, axis=axis))
    return d if guide.ndim == 2 else d.max(axis=2)


def solve_lines(xs, w, lam):
    """One pass of step 4 over L lines at once.  xs: arrays (L, n), the right-hand sides that share the coefficients; w: (L, n - 1)
    weights; lam: lambda_t as a scalar of the arrays' dtype.  Returns the solutions, same shapes."""
    dt = xs[0].dtype.type
    L, n = xs[0].shape
    if n == 1:
        return [x.copy() for x in xs]
    one = dt(1)
    k = lam * w
    cp = np.empty((L, n), dt)
    xp = [np.empty((L, n), dt) for _ in xs]
    c = -k[:, 0]
    b = (one - np.zeros(L, dt)) - c
    r = one / b
    cp[:, 0] = c * r
    for p, x in zip(xp, xs):
        p[:, 0] = x[:, 0] * r
    zero = np.zeros(L, dt)
    for i in range(1, n):
        a = -k[:, i - 1]
        c = -k[:, i] if i < n - 1 else zero
        b = (one - a) - c
        m = b - a * cp[:, i - 1]
        r = one / m
        cp[:, i] = c * r
        for p, x in zip(xp, xs):
            p[:, i] = (x[:, i] - a * p[:, i - 1]) * r
    out = [np.empty((L, n), dt) for _ in xs]
    for o, p in zip(out, xp):
        o[:, n - 1] = p[:, n - 1]
        for i in range(n - 2, -1, -1):
            o[:, i] = p[:, i] - cp[:, i] * o[:, i + 1]
    return out


def wls_filter(disp, guide, conf, invalid, lam, lut, dtype=np.float32, T=T_DEFAULT):
    """Returns dict(out int16, out_f32, q (u / v, 0 where invalid), valid, u, v).  lut: the 256 float32 weights."""
    dt = np.dtype(dtype).type
    disp = np.asarray(disp)
    assert disp.dtype == np.int16 and disp.ndim == 2 and guide.dtype == np.uint8 and guide.shape[:2] == disp.shape
    ok = disp != invalid
    c = np.where(ok, dt(100) if conf is None else conf.astype(dt), dt(0)).astype(dt)
    u = np.where(ok, disp.astype(dt) * c, dt(0)).astype(dt)
    v = c.copy()
    lut = np.asarray(lut, np.float32).astype(dt)
    wr = lut[edge_index(guide, 1)]              # (H, W - 1)
    wc = lut[edge_index(guide, 0)].T.copy()     # (W, H - 1): the lines of a column pass
    with np.errstate(all="ignore"):
        for lt in lambdas(lam, T):
            u, v = solve_lines([u, v], wr, dt(lt))
            ut, vt = solve_lines([np.ascontiguousarray(u.T), np.ascontiguousarray(v.T)], wc, dt(lt))
            u, v = np.ascontiguousarray(ut.T), np.ascontiguousarray(vt.T)
        valid = v >= dt(1)
        q = np.divide(u, v, out=np.zeros_like(u), where=valid)
        out = np.where(valid, np.clip(np.rint(q), -32768, 32767), invalid).astype(np.int16)
        out_f = np.where(valid, q * dt(0.0625), dt(0)).astype(dt)
    return dict(out=out, out_f32=out_f, q=q, valid=valid, u=u, v=v)


def layered_scene(H, W, seed):
    """A scene whose grey levels follow its depth layers: disparity layers 200 / 420 / 600 with guide levels 60 / 120 / 180 +- 2
    behind slanted boundaries; the map carries +-24 of noise, 5 % outliers (any value in 0 .. 800, confidence below 15; the
    others 40 .. 100) and 20 % holes.  Returns dict(truth, disp, guide, conf, invalid)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    layer = (xx + yy // 3 >= W // 3).astype(int) + (xx - yy // 4 >= 2 * W // 3).astype(int)
    truth = np.array([200, 420, 600], np.int16)[layer]
    guide = (np.array([60, 120, 180])[layer] + rng.integers(-2, 3, (H, W))).astype(np.uint8)
    disp = (truth + rng.integers(-24, 25, (H, W))).astype(np.int16)
    conf = rng.integers(40, 101, (H, W)).astype(np.uint8)
    outl = rng.random((H, W)) < 0.05
    disp[outl] = rng.integers(0, 801, int(outl.sum())).astype(np.int16)
    conf[outl] = rng.integers(1, 15, int(outl.sum())).astype(np.uint8)
    invalid = -16
    hole = rng.random((H, W)) < 0.20
    disp[hole] = invalid
    return dict(truth=truth, disp=disp, guide=guide, conf=conf, invalid=invalid)


# ---- inputs of the device tests (tests/test_gpu_wls.py, tests/wls_guard_child.py) -----------------------------------------------
def random_input(H, W, cn=1, seed=0, invalid=-16, holes=0.3, with_conf=True):
    """A map in blocks of 8 x 8 with noise and holes, a guide in blocks of its own with noise (so that weights of every size
    occur, within a block and across its edges), a confidence map over the whole of 0 .. 100.  With invalid = -160 the map holds
    negative disparities as a matcher with minDisparity = -9 returns them."""
    rng = np.random.default_rng([seed, H, W, cn])
    by, bx = (H + 7) // 8, (W + 7) // 8
    up = lambda a: np.kron(a, np.ones((8, 8), a.dtype))[:H, :W]
    disp = (up(rng.integers(invalid + 16, 1800, (by, bx))) + rng.integers(-20, 21, (H, W))).astype(np.int16)
    disp[disp == invalid] += 1
    disp[rng.random((H, W)) < holes] = invalid
    shape = (H, W) if cn == 1 else (H, W, 3)
    lvl = up(rng.integers(0, 5, (by, bx)) * 50)
    guide = ((lvl if cn == 1 else lvl[:, :, None]) + rng.integers(0, 7, shape)).astype(np.uint8)
    conf = rng.integers(0, 101, (H, W)).astype(np.uint8) if with_conf else None
    return dict(disp=disp, guide=guide, conf=conf, invalid=invalid)


# (H, W, cn, with_conf, lambda, sigma, invalid): degenerate lines; tile edges of the row kernel; three row-waves with a partial
# tile; more than one wave of columns -- crossed sparingly with the channel count, the confidence map, lambda / sigma and the
# invalid value
SHAPE_CASES = [(1, 1, 1, True, 8000.0, 1.5, -16), (1, 7, 3, False, 8000.0, 1.5, -16), (7, 1, 1, True, 100.0, 10.0, -160),
               (2, 2, 3, True, 8000.0, 0.5, -16), (5, 63, 1, False, 1e6, 1.5, -16), (64, 64, 3, True, 8000.0, 1.5, -160),
               (65, 129, 1, True, 8000.0, 1.5, -16), (130, 67, 3, False, 100.0, 10.0, -16), (200, 33, 1, True, 8000.0, 0.5, -160),
               (97, 260, 3, True, 1e6, 1.5, -16)]
