"""The statistical outlier removal of include/sgm_hip_statistical.h, restated in numpy, twice: over all pairs (`brute`, in chunks)
and over the 27 cells around each point of the cloud sorted by cell (`cells`, for larger clouds) -- the reference the device
results are held against bit for bit (tests/test_gpu_statistical.py), the hand-worked answers of
tests/test_statistical_reference.py and the case table.  Validity, the host constants, the range rule, the distance and the cloud
generators are those of tests/radius_ref.py, imported, not copied.  Nothing here knows about a hash table, a probe, a register
list or an arrival order; every float step is one numpy float32 operation, rounded to binary32 on its own, and the threshold is
formed in Python floats (binary64), one operation at a time."""
import math

import numpy as np

import radius_ref as RR
from radius_ref import classify, constants, d2_of, face_pairs, lattice, layered_lists, random_list  # noqa: F401  (the tests' generators)

MAX_K = 64
F32 = np.float32
INF = F32(np.inf)
STATS = ("in_range", "out_of_range", "dense", "sparse", "A", "B", "T")


def qscale_of(radius):
    """the one more host constant of steps 1 - 4"""
    constants(radius)
    with np.errstate(all="ignore"):
        qs = F32(524288.0) / F32(radius)
    assert np.isfinite(qs)
    return qs


def means_of(near_d2, k):
    """steps 5 and 6 on a matrix of d2 values, one row per point, with +inf wherever there is no neighbour: (c, dense, mean), mean
    meaningful on the dense rows"""
    rows = near_d2.shape[0]
    c = (near_d2 < INF).sum(axis=1)
    dense = c >= k
    mean = np.full(rows, -1, np.float32)
    if dense.any():
        D = near_d2[dense]
        if D.shape[1] > k:
            D = np.partition(D, k - 1, axis=1)[:, :k]          # the k smallest, as values
        s = np.sqrt(np.sort(D, axis=1))                        # float32 in, float32 out: the correctly rounded root
        assert s.dtype == np.float32
        acc = s[:, 0].copy()
        for m in range(1, k):
            acc = acc + s[:, m]                                # ascending, one binary32 addition each
        mean[dense] = acc / F32(k)
    return c, dense, mean


def threshold(m, A, B, std_ratio):
    """step 8: Python floats are binary64 and every operation below rounds on its own"""
    if m == 0:
        return 0
    mu = float(A) / float(m)
    var = (float(B) - float(A) * mu) / float(m - 1) if m >= 2 else 0.0
    if var < 0.0:
        var = 0.0
    thr = mu + float(F32(std_ratio)) * math.sqrt(var)
    return min(int(math.floor(thr)), 2 ** 32 - 2)


def _finish(xyz, colors, valid, inr, dense_all, mean_all, k, std_ratio, radius):
    """steps 7 to 10 from the per-point means"""
    n = xyz.shape[0]
    qs = qscale_of(radius)
    q = np.zeros(n, np.uint32)
    with np.errstate(all="ignore"):
        q[dense_all] = (mean_all[dense_all] * qs).astype(np.uint32)       # one binary32 product, then truncation
    qd = [int(x) for x in q[dense_all]]
    m, A, B = len(qd), sum(qd), sum(x * x for x in qd)                   # Python integers: exact
    assert B < 2 ** 63
    T = threshold(m, A, B, std_ratio)
    keep = (dense_all & (q <= T)).astype(np.uint8)
    idx = np.nonzero(keep)[0]
    if colors is not None:
        colors = np.asarray(colors)
        assert colors.dtype == np.uint8 and colors.shape == (n, 3)
    n_in = int(inr.sum())
    stats = np.array([n_in, int((valid & ~inr).sum()), m, n_in - m, A, B, T, 0], np.uint64)
    return dict(keep=keep, mean=np.where(dense_all, mean_all, F32(-1)).astype(np.float32), points=xyz[idx],
                colors=None if colors is None else colors[idx], index=idx.astype(np.uint32), n_kept=int(idx.size), stats=stats,
                q=q, dense=dense_all, in_range=inr)


def _check(xyz, k, std_ratio):
    assert xyz.shape[0] <= RR.MAX_POINTS and 1 <= k <= MAX_K
    assert np.isfinite(F32(std_ratio)) and F32(std_ratio) >= 0


def brute(xyz, disp=None, colors=None, nb_neighbors=8, std_ratio=1.0, max_radius=0.02, origin=(0.0, 0.0, 0.0), chunk=512):
    """The whole definition over all pairs.  Returns a dict: keep uint8 (n), mean float32 (n), points, colors, index uint32,
    n_kept, stats uint64 (8), and for the tests q uint32 (n), dense and in_range."""
    xyz = np.asarray(xyz)
    n, k = xyz.shape[0], int(nb_neighbors)
    _check(xyz, k, std_ratio)
    r2, _, _ = constants(max_radius)
    valid, inr, _ = classify(xyz, disp, max_radius, origin)
    ids = np.nonzero(inr)[0]
    P = xyz[ids]
    dense_all, mean_all = np.zeros(n, bool), np.full(n, -1, np.float32)
    for lo in range(0, ids.size, chunk):
        A = P[lo:lo + chunk]
        with np.errstate(all="ignore"):
            d2 = d2_of(A[:, None, :], P[None, :, :])
        d2 = np.where(d2 <= r2, d2, INF)
        d2[np.arange(A.shape[0]), lo + np.arange(A.shape[0])] = INF      # j != i
        _, dense, mean = means_of(d2, k)
        dense_all[ids[lo:lo + chunk]] = dense
        mean_all[ids[lo:lo + chunk]] = mean
    return _finish(xyz, colors, valid, inr, dense_all, mean_all, k, std_ratio, max_radius)


def cells(xyz, disp=None, colors=None, nb_neighbors=8, std_ratio=1.0, max_radius=0.02, origin=(0.0, 0.0, 0.0), budget=1 << 21):
    """The same through the cells: the points sorted by cell key, and per point the candidates of its 27 neighbour cells (those
    inside the index range), a block of points at a time (at most `budget` candidate pairs, one point more where a single point
    has more)."""
    xyz = np.asarray(xyz)
    n, k = xyz.shape[0], int(nb_neighbors)
    _check(xyz, k, std_ratio)
    r2, _, _ = constants(max_radius)
    valid, inr, gi = classify(xyz, disp, max_radius, origin)
    ids = np.nonzero(inr)[0]
    dense_all, mean_all = np.zeros(n, bool), np.full(n, -1, np.float32)
    if ids.size:
        key = RR.key_of(gi[ids])
        order = np.argsort(key, kind="stable")
        ids, key, g = ids[order], key[order], gi[ids][order]
        P = xyz[ids]
        m = ids.size
        lo = np.zeros((27, m), np.int64)
        ln = np.zeros((27, m), np.int64)
        for o, off in enumerate(RR.OFFSETS):
            ng = g + off[None, :]
            ok = ((ng >= -RR.G_BIAS) & (ng < RR.G_BIAS)).all(axis=1)
            nk = RR.key_of(np.where(ok[:, None], ng, 0))
            lo[o] = np.searchsorted(key, nk, side="left")
            ln[o] = np.where(ok, np.searchsorted(key, nk, side="right") - lo[o], 0)
        per_point = ln.sum(axis=0)
        ends = np.cumsum(per_point)
        a = 0
        while a < m:
            b = max(a + 1, int(np.searchsorted(ends, (ends[a - 1] if a else 0) + budget, side="right")))
            width = int(per_point[a:b].max())
            D = np.full((b - a, max(width, 1)), INF, np.float32)
            col0 = np.zeros(b - a, np.int64)
            for o in range(27):
                L = ln[o, a:b]
                tot = int(L.sum())
                if tot:
                    i = np.repeat(np.arange(a, b), L)
                    first = np.repeat(np.cumsum(L) - L, L)
                    within = np.arange(tot) - first
                    j = np.repeat(lo[o, a:b], L) + within
                    with np.errstate(all="ignore"):
                        d2 = d2_of(P[i], P[j])
                    D[i - a, np.repeat(col0, L) + within] = np.where((d2 <= r2) & (i != j), d2, INF)
                col0 += L
            _, dense, mean = means_of(D, k)
            dense_all[ids[a:b]] = dense
            mean_all[ids[a:b]] = mean
            a = b
    return _finish(xyz, colors, valid, inr, dense_all, mean_all, k, std_ratio, max_radius)


# ---- the case table ------------------------------------------------------------------------------------------------------------
# (kind, a, b, nb_neighbors, std_ratio, max_radius, origin).  kind "list": radius_ref.random_list(a, seed 900 + b, extent 0.5);
# "layered": the layered cloud a x b of radius_ref.  The kernels work in blocks of 256 points and waves of 64: 63 under one wave,
# 64 exactly one, 65 and 257 ragged.  The lists' k and radii give dense and sparse points wherever the list has enough points.
SHAPE_CASES = [
    ("list", 1, 0, 1, 1.0, 0.1, (0.0, 0.0, 0.0)),
    ("list", 2, 1, 1, 1.0, 0.9, (0.0, 0.0, 0.0)),
    ("list", 63, 2, 2, 1.0, 0.15, (0.0, 0.0, 0.0)),
    ("list", 64, 3, 1, 0.5, 0.12, (0.0, 0.0, 0.0)),
    ("list", 65, 4, 3, 1.0, 0.2, (0.25, -0.5, 0.125)),
    ("list", 257, 5, 4, 1.0, 0.11, (0.0, 0.0, 0.0)),
    ("layered", 24, 130, 4, 1.0, 0.03, (0.0, 0.0, 0.0)),
    ("layered", 48, 320, 8, 1.0, 0.02, (0.0, 0.0, 0.0)),
    ("layered", 48, 320, 16, 0.5, 0.04, (-0.5, 0.25, 1.0)),
    ("layered", 48, 320, 4, 1.0, 0.03, (0.0, 0.0, 0.0)),
]

# the kept-share rows: (H, W, seed, r, k, ratio, dense, sparse, kept, T)
SHARE_ROWS = [
    (48, 320, 704, 0.03, 4, 1.0, 13553, 23, 11377, 257970),
    (48, 320, 704, 0.02, 8, 1.0, 9094, 4482, 7436, 348650),
    (48, 320, 704, 0.04, 16, 0.5, 13451, 125, 8946, 250929),
    (24, 130, 724, 0.03, 4, 1.0, 1771, 974, 1464, 386084),
    (24, 130, 724, 0.04, 16, 2.0, 1169, 1576, 1087, 390929),
]
SPARSE_ROW = (24, 130, 724, 0.02, 8, 1.0, 59, 2686, 49)      # the sparse-dominated row: dense, sparse, kept (no share condition)


def case_input(i):
    kind, a, b = SHAPE_CASES[i][:3]
    if kind == "list":
        xyz, col = random_list(a, 900 + b, 0.5)
        return xyz, None, col
    return layered_lists(a, b, 704 if (a, b) == (48, 320) else 700 + a)


_cache = {}


def shared(key, make):
    """a reference computed once and shared, its arrays read-only"""
    if key not in _cache:
        res = make()
        for a in res.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = res
    return _cache[key]


def case_want(i, with_disp=True):
    """the reference of shape case i (the cell form)"""
    def make():
        k, ratio, r, o = SHAPE_CASES[i][3:]
        xyz, disp, col = case_input(i)
        return cells(xyz, disp if with_disp else None, col, k, ratio, r, o)
    return shared(("case", i, with_disp), make)


def layered_want(H, W, seed, k, ratio, r, origin=(0.0, 0.0, 0.0)):
    """the reference on a layered cloud with disparities and colours"""
    return shared(("layered", H, W, seed, k, ratio, r, tuple(origin)), lambda: cells(*layered_lists(H, W, seed), k, ratio, r, origin))
