"""The left-right consistency confidence of include/sgm_hip_lrc.h, restated in numpy: the reference the device results are held
against bit for bit (tests/test_gpu_lrc.py), the hand-worked answers of tests/test_lrc_reference.py, the input generator and the
shape list.  The windows are formed DIRECTLY -- one shifted copy of the map per window position, not the separable sums the
kernel uses -- in int64, and every product of the definition is bounded with Python integers, so a result that depended on
int64 wrapping would fail here before it could agree with the device."""
import numpy as np

I64_MAX = (1 << 63) - 1
T_DEFAULT, V_DEFAULT = 24, 2304


def smoothness(M, invalid, r, V):
    """F_M of the definition, step 1: uint8 (H, W)"""
    M = np.asarray(M)
    assert M.dtype == np.int16 and M.ndim == 2 and 0 <= r <= 16 and 1 <= V <= 1 << 30
    H, W = M.shape
    v = M.astype(np.int64)
    ok = M != invalid
    pv = np.zeros((H + 2 * r, W + 2 * r), np.int64)
    pk = np.zeros((H + 2 * r, W + 2 * r), np.int64)
    pv[r:r + H, r:r + W] = np.where(ok, v, 0)
    pk[r:r + H, r:r + W] = ok
    n, s1, s2 = (np.zeros((H, W), np.int64) for _ in range(3))
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            a, k = pv[dy:dy + H, dx:dx + W], pk[dy:dy + H, dx:dx + W]
            n += k
            s1 += a
            s2 += a * a          # (at most 2^30 each, at most 33^2 of them)
    # no intermediate leaves int64: each product is bounded by the product of its factors' largest magnitudes
    nmax, s1max, s2max = int(n.max()), int(np.abs(s1).max()), int(s2.max())
    assert nmax * s2max <= I64_MAX and s1max * s1max <= I64_MAX, (nmax, s1max, s2max)
    assert 100 * nmax * s2max <= I64_MAX and nmax * nmax * int(V) <= I64_MAX, (nmax, s2max, V)
    num = n * s2 - s1 * s1
    assert int(num.min()) >= 0
    den = np.maximum(n, 1) ** 2 * np.int64(V)
    q = (100 * num) // den       # (both non-negative: floor division is C's)
    F = 100 - np.minimum(100, q)
    return np.where(ok, F, 0).astype(np.uint8)


def _one(d_own, d_other, F_own, F_other, base, sign, invalid, T, base_at_other):
    H, W = d_own.shape
    d = d_own.astype(np.int64)
    x = np.arange(W, dtype=np.int64)[None, :]
    xo = x + sign * np.floor_divide(d + 8, 16)
    inside = (xo >= 0) & (xo < W)
    xc = np.clip(xo, 0, W - 1)
    rows = np.arange(H)[:, None]
    e = d_other.astype(np.int64)[rows, xc]
    good = (d_own != invalid) & inside & (d_other[rows, xc] != invalid) & (np.abs(d - e) <= T)
    c = np.minimum(F_own.astype(np.int64), F_other.astype(np.int64)[rows, xc])
    if base is not None:
        b = base.astype(np.int64)
        c = np.minimum(c, b[rows, xc] if base_at_other else b)
    return np.where(good, c, 0).astype(np.uint8)


def lrc_confidence(dl, dr, base=None, invalid=-16, thresh=T_DEFAULT, radius=5, var_max=V_DEFAULT):
    """(conf_left, conf_right) of the definition, steps 2 and 3: uint8 (H, W) each"""
    dl, dr = np.asarray(dl), np.asarray(dr)
    assert dl.dtype == np.int16 and dr.dtype == np.int16 and dl.shape == dr.shape and dl.ndim == 2
    assert -32768 <= invalid <= 32767 and 0 <= thresh <= 32767
    if base is not None:
        base = np.asarray(base)
        assert base.dtype == np.uint8 and base.shape == dl.shape
    Fl, Fr = smoothness(dl, invalid, radius, var_max), smoothness(dr, invalid, radius, var_max)
    left = _one(dl, dr, Fl, Fr, base, -1, invalid, thresh, False)
    right = _one(dr, dl, Fr, Fl, base, +1, invalid, thresh, True)      # (base lives in the left view: read at the match)
    return left, right


def random_pair(H, W, seed, invalid=-16, levels=None, holes=0.10, outliers=0.05):
    """A left map of piecewise-constant levels with noise, the right map its forward warp with noise of its own, outliers and
    holes, and a random base.  levels: sixteenths above invalid + 16, one per 16 x 32 block (2 x 32 when H <= 8); by default 0 / 8 / 20 / 40 / 64, and
    0 alone when W <= 8 (so that narrow maps keep matches inside the image)."""
    rng = np.random.default_rng(seed)
    if levels is None:
        levels = (0,) if W <= 8 else (0, 8, 20, 40, 64)
    zero = invalid + 16
    bh = 16 if H > 8 else 2                  # (short maps hold more than one level)
    by, bx = (H + bh - 1) // bh, (W + 31) // 32
    lev = rng.choice(np.asarray(levels), size=(by, bx))
    dl = zero + np.kron(lev, np.ones((bh, 32), np.int64))[:H, :W] + rng.integers(-6, 7, size=(H, W))
    dr = np.full((H, W), invalid, np.int64)
    xr = np.arange(W)[None, :] - np.floor_divide(dl + 8, 16)
    noise = rng.integers(-4, 5, size=(H, W))
    for y in range(H):
        for x in range(W):          # (later left pixels overwrite earlier ones: any of them will do)
            if 0 <= xr[y, x] < W:
                dr[y, xr[y, x]] = dl[y, x] + noise[y, x]
    out = rng.random((H, W)) < outliers
    dr[out] = rng.integers(zero - 100, zero + 200, size=int(out.sum()))
    dl[rng.random((H, W)) < holes] = invalid
    dr[rng.random((H, W)) < holes] = invalid
    base = rng.integers(0, 101, size=(H, W)).astype(np.uint8)
    assert dl.min() >= -32768 and dl.max() <= 32767 and dr.min() >= -32768 and dr.max() <= 32767
    return dict(dl=dl.astype(np.int16), dr=dr.astype(np.int16), base=base)


def extreme_pair(H, W, invalid=-16):
    """maps alternating -32768 / 32767: the largest sums the definition can meet"""
    m = np.where((np.add.outer(np.arange(H), np.arange(W)) & 1) == 0, -32768, 32767).astype(np.int16)
    return dict(dl=m, dr=m[:, ::-1].copy(), base=np.full((H, W), 100, np.uint8))


# (H, W, radius, thresh, var_max, invalid, levels): the shapes of the issue, then what straddles the tiles of the kernels as
# built -- k_lrc_factor works in tiles of 64 x 16 pixels with an r-wide halo, k_lrc_match in row pieces of 256 pixels:
#   16 x 64    exactly one tile;   17 x 65   one pixel into the next tile on both axes;   15 x 63   one short of a tile;
#   32 x 128   whole tiles only, r = 16: every halo reaches into a neighbour tile and past the image;
#   3 x 257    one pixel into the second row piece of k_lrc_match;   18 x 256   exactly one row piece, two tile rows
SHAPE_CASES = [
    (1, 1, 16, 24, 2304, -16, None),
    (1, 7, 5, 24, 2304, -16, None),
    (7, 1, 5, 24, 2304, -16, (0, 20, 64)),          # disparities that leave the image
    (5, 63, 0, 0, 2304, -16, None),
    (64, 64, 4, 24, 2304, -16, None),
    (65, 129, 6, 24, 2304, -16, None),
    (33, 200, 16, 8, 1024, -16, None),              # window taller than half the image
    (97, 260, 1, 24, 64, -16, None),
    (130, 67, 5, 24, 2304, -160, None),
    (200, 33, 5, 24, 2304, -16, None),
    (16, 64, 3, 24, 2304, -16, None),
    (17, 65, 3, 24, 2304, -160, None),
    (15, 63, 2, 24, 2304, -16, None),
    (32, 128, 16, 24, 2304, -16, None),
    (3, 257, 2, 24, 2304, -16, None),
    (18, 256, 7, 24, 2304, -16, None),
]


def case_input(i):
    H, W, r, T, V, invalid, levels = SHAPE_CASES[i]
    return random_pair(H, W, 500 + i, invalid, levels)


_cache = {}


def case_want(i, with_base=True):
    """the reference of shape case i, computed once and shared (read-only)"""
    key = (i, with_base)
    if key not in _cache:
        H, W, r, T, V, invalid, levels = SHAPE_CASES[i]
        s = case_input(i)
        cl, cr = lrc_confidence(s["dl"], s["dr"], s["base"] if with_base else None, invalid, T, r, V)
        cl.setflags(write=False)
        cr.setflags(write=False)
        _cache[key] = (cl, cr)
    return _cache[key]
