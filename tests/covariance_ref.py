"""The covariance normals of include/sgm_hip_covariance.h, restated in numpy, twice: over all pairs (`brute`, in chunks) and over
the 27 cells around each point of the cloud sorted by cell (`cells`, for larger clouds) -- the reference the device results are
held against bit for bit (tests/test_gpu_covariance.py), the hand-worked answers of tests/test_covariance_reference.py and the
case table.  Validity, the host constants, the range rule, the distance and the cloud generators are those of tests/radius_ref.py,
imported, not copied.  Nothing here knows about a hash table, a probe or an arrival order; every binary32 step is one numpy float32
operation, the nine sums are np.int64, and steps 7 to 10 are Python floats (binary64) and math.sqrt, one operation per line."""
import functools
import math

import numpy as np

import radius_ref as RR
from radius_ref import classify, constants, d2_of, face_pairs, layered_lists, random_list  # noqa: F401  (the tests' generators)

MIN_K = 2
F32 = np.float32
STATS = ("in_range", "out_of_range", "with_normal", "degenerate")
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))       # the order of the six second moments


def qscale_of(radius):
    """the one more host constant of steps 1 - 4"""
    constants(radius)
    with np.errstate(all="ignore"):
        qs = F32(32768.0) / F32(radius)
    assert np.isfinite(qs)
    return qs


def quantise(d, near, qs):
    """step 6 for float32 offsets d (..., 3) of the pairs `near`: int64 (..., 3), zero where not near"""
    assert d.dtype == np.float32
    with np.errstate(all="ignore"):
        prod = d * qs                                              # one binary32 product
    assert prod.dtype == np.float32
    return np.rint(np.where(near[..., None], prod, F32(0))).astype(np.int64)      # to nearest, ties to even


def jacobi(a, sweeps=6):
    """step 8 on the symmetric matrix a (six floats a00 a01 a02 a11 a12 a22): (diagonal, V as rows, off-diagonals)"""
    A = [[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]]      # only A[p][q] with p <= q is kept up to date
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    get = lambda i, j: A[min(i, j)][max(i, j)]

    def put(i, j, x):
        A[min(i, j)][max(i, j)] = x
    for _ in range(sweeps):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = get(p, q)
            if apq == 0.0:
                continue
            diff = get(q, q) - get(p, p)
            twice = 2.0 * apq
            theta = diff / twice
            sq = theta * theta
            sq1 = sq + 1.0
            root = math.sqrt(sq1)
            den = abs(theta) + root
            sgn = 1.0 if theta >= 0.0 else -1.0
            t = sgn / den
            tt = t * t
            tt1 = tt + 1.0
            c = 1.0 / math.sqrt(tt1)
            sn = t * c
            h = t * apq
            put(p, p, get(p, p) - h)
            put(q, q, get(q, q) + h)
            put(p, q, 0.0)
            arp, arq = get(r, p), get(r, q)
            c_arp = c * arp
            sn_arq = sn * arq
            sn_arp = sn * arp
            c_arq = c * arq
            put(r, p, c_arp - sn_arq)
            put(r, q, sn_arp + c_arq)
            for row in V:
                vp, vq = row[p], row[q]
                c_vp = c * vp
                sn_vq = sn * vq
                sn_vp = sn * vp
                c_vq = c * vq
                row[p] = c_vp - sn_vq
                row[q] = sn_vp + c_vq
    return [A[0][0], A[1][1], A[2][2]], V, [A[0][1], A[0][2], A[1][2]]


def covariance(S, m):
    """step 7: the six C_ab from the nine integer sums, and the matrix divided by its largest diagonal entry (None: degenerate)"""
    d = [float(int(x)) for x in S[:3]]            # int -> binary64, to nearest even
    C = []
    for (a, b), sab in zip(PAIRS, S[3:]):
        prod = d[a] * d[b]
        quot = prod / float(m)
        C.append(float(int(sab)) - quot)
    s = max(C[0], C[3], C[5])
    if not s > 0.0:
        return C, None
    return C, [x / s for x in C]


@functools.lru_cache(maxsize=1 << 16)
def _solve(S, m):
    """steps 7 to 10 without the orientation: None for a degenerate point, else ((n0, n1, n2) binary64, kappa binary64, i*)"""
    _, A = covariance(S, m)
    if A is None:
        return None
    lam, V, _ = jacobi(A)
    i = 0
    if lam[1] < lam[i]:
        i = 1
    if lam[2] < lam[i]:
        i = 2
    n0, n1, n2 = V[0][i], V[1][i], V[2][i]
    s01 = n0 * n0 + n1 * n1
    len2 = s01 + n2 * n2
    ln = math.sqrt(len2)
    n0, n1, n2 = n0 / ln, n1 / ln, n2 / ln
    l0, l1, l2 = max(lam[0], 0.0), max(lam[1], 0.0), max(lam[2], 0.0)
    den = (l0 + l1) + l2
    kappa = 0.0 if den == 0.0 else max(lam[i], 0.0) / den
    return (n0, n1, n2), kappa, i


def solve(S, c, p, viewpoint=(0.0, 0.0, 0.0), orient=True):
    """steps 7 to 10 for one point with c neighbours: (normal float32 (3), kappa float32, degenerate)"""
    got = _solve(tuple(int(x) for x in S), int(c) + 1)
    if got is None:
        return np.zeros(3, np.float32), F32(-1), True
    (n0, n1, n2), kappa, _ = got
    if orient:
        w0 = float(F32(p[0])) - float(F32(viewpoint[0]))
        w1 = float(F32(p[1])) - float(F32(viewpoint[1]))
        w2 = float(F32(p[2])) - float(F32(viewpoint[2]))
        dot = (n0 * w0 + n1 * w1) + n2 * w2
        if dot > 0.0:
            n0, n1, n2 = -n0, -n1, -n2
    return np.array([n0, n1, n2], np.float64).astype(np.float32), F32(kappa), False


def _finish(xyz, valid, inr, c, S, k, viewpoint, orient):
    """steps 7 to 11 from the per-point counts and sums"""
    n = xyz.shape[0]
    assert MIN_K <= k <= RR.MAX_POINTS and np.isfinite(np.asarray(viewpoint, np.float32)).all()
    nrm = np.zeros((n, 3), np.float32)
    kap = np.full(n, -1, np.float32)
    has = np.zeros(n, bool)
    deg = np.zeros(n, bool)
    for i in np.nonzero(inr & (c >= k))[0]:
        nrm[i], kap[i], deg[i] = solve(S[i], c[i], xyz[i], viewpoint, orient)
        has[i] = not deg[i]
    n_in = int(inr.sum())
    stats = np.array([n_in, int((valid & ~inr).sum()), int(has.sum()), int(deg.sum())], np.uint64)
    return dict(normals=nrm, curvature=kap, counts=c.astype(np.uint32), stats=stats, moments=S, has_normal=has, degenerate=deg, in_range=inr)


def brute(xyz, disp=None, radius=0.02, min_neighbors=3, origin=(0.0, 0.0, 0.0), viewpoint=(0.0, 0.0, 0.0), orient=True, chunk=256):
    """The whole definition over all pairs.  Returns a dict: normals float32 (n, 3), curvature float32 (n), counts uint32 (n),
    stats uint64 (4), and for the tests moments int64 (n, 9), has_normal, degenerate and in_range."""
    xyz = np.asarray(xyz)
    n = xyz.shape[0]
    assert n <= RR.MAX_POINTS
    r2, _, _ = constants(radius)
    qs = qscale_of(radius)
    valid, inr, _ = classify(xyz, disp, radius, origin)
    ids = np.nonzero(inr)[0]
    P = xyz[ids]
    c = np.zeros(n, np.int64)
    S = np.zeros((n, 9), np.int64)
    for lo in range(0, ids.size, chunk):
        A = P[lo:lo + chunk]
        with np.errstate(all="ignore"):
            d = P[None, :, :] - A[:, None, :]                       # x_j - x_i: the differences of step 4
            near = d2_of(A[:, None, :], P[None, :, :]) <= r2
        near[np.arange(A.shape[0]), lo + np.arange(A.shape[0])] = False      # j != i
        q = quantise(d, near, qs)
        rows = ids[lo:lo + chunk]
        c[rows] = near.sum(axis=1)
        S[rows, :3] = q.sum(axis=1)
        for w, (a, b) in enumerate(PAIRS):
            S[rows, 3 + w] = (q[..., a] * q[..., b]).sum(axis=1)
    return _finish(xyz, valid, inr, c, S, int(min_neighbors), viewpoint, orient)


def cells(xyz, disp=None, radius=0.02, min_neighbors=3, origin=(0.0, 0.0, 0.0), viewpoint=(0.0, 0.0, 0.0), orient=True, budget=1 << 21):
    """The same through the cells: the points sorted by cell key, and per point the candidates of its 27 neighbour cells (those
    inside the index range), expanded `budget` candidate pairs at a time."""
    xyz = np.asarray(xyz)
    n = xyz.shape[0]
    assert n <= RR.MAX_POINTS
    r2, _, _ = constants(radius)
    qs = qscale_of(radius)
    valid, inr, gi = classify(xyz, disp, radius, origin)
    ids = np.nonzero(inr)[0]
    c = np.zeros(n, np.int64)
    S = np.zeros((n, 9), np.int64)
    if ids.size:
        key = RR.key_of(gi[ids])
        order = np.argsort(key, kind="stable")
        ids, key, g = ids[order], key[order], gi[ids][order]
        P = xyz[ids]
        m = ids.size
        cs = np.zeros(m, np.int64)
        Ss = np.zeros((m, 9), np.int64)
        for off in RR.OFFSETS:
            ng = g + off[None, :]
            ok = ((ng >= -RR.G_BIAS) & (ng < RR.G_BIAS)).all(axis=1)
            nk = RR.key_of(np.where(ok[:, None], ng, 0))
            lo = np.searchsorted(key, nk, side="left")
            ln = np.where(ok, np.searchsorted(key, nk, side="right") - lo, 0)
            ends = np.cumsum(ln)
            a = 0
            while a < m:       # points a .. b - 1: at most `budget` pairs (one point more where a single point has more)
                b = max(a + 1, int(np.searchsorted(ends, (ends[a - 1] if a else 0) + budget, side="right")))
                L = ln[a:b]
                tot = int(L.sum())
                if tot:
                    i = np.repeat(np.arange(a, b), L)
                    first = np.repeat(np.cumsum(L) - L, L)
                    j = np.repeat(lo[a:b], L) + (np.arange(tot) - first)
                    with np.errstate(all="ignore"):
                        near = (d2_of(P[i], P[j]) <= r2) & (i != j)
                        i, j = i[near], j[near]
                        d = P[j] - P[i]
                    q = quantise(d, np.ones(i.size, bool), qs)
                    cs[a:b] += np.bincount(i - a, minlength=b - a)
                    np.add.at(Ss[:, :3], i, q)
                    for w, (u, v) in enumerate(PAIRS):
                        np.add.at(Ss[:, 3 + w], i, q[:, u] * q[:, v])
                a = b
        c[ids] = cs
        S[ids] = Ss
    return _finish(xyz, valid, inr, c, S, int(min_neighbors), viewpoint, orient)


def max_abs_q(xyz, radius, origin=(0.0, 0.0, 0.0), chunk=256):
    """the bound of step 6, measured over all pairs: the largest |q_a| among the neighbours (-1 if there is no pair)"""
    r2, _, _ = constants(radius)
    qs = qscale_of(radius)
    _, inr, _ = classify(xyz, None, radius, origin)
    P = xyz[inr]
    worst = -1
    for lo in range(0, P.shape[0], chunk):
        A = P[lo:lo + chunk]
        with np.errstate(all="ignore"):
            d = P[None, :, :] - A[:, None, :]
            near = d2_of(A[:, None, :], P[None, :, :]) <= r2
        if near.any():
            worst = max(worst, int(np.abs(quantise(d, near, qs)).max()))
    return worst


def plane_lattice(H, W, spacing=0.25, z=2.0, x0=-3.0, y0=-1.0, slope=0.0):
    """H x W points of a square lattice in the plane Z = z + slope * X' (X' the lattice abscissa), spacing a power of two: with
    r = 1.5 * spacing every offset is 0 or +-spacing and quantises exactly (to 0 or +-2^15 / 1.5 rounded -- see the tests)"""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    X = xx * F32(spacing)
    out = np.stack([X + F32(x0), yy * F32(spacing) + F32(y0), F32(z) + F32(slope) * X], axis=2).reshape(-1, 3).astype(np.float32)
    return out


# ---- the case table ------------------------------------------------------------------------------------------------------------
# (kind, a, b, radius, min_neighbors, origin, viewpoint, orient).  kind "list": radius_ref.random_list(a, seed 900 + b, extent 0.5);
# "layered": the first a points of the in-range part of the 24 x 130 layered cloud (b = 0), or the whole a x b layered cloud as an
# XYZ image with its disparities.  The kernels work in blocks of 256 points and waves of 64: 63 under one wave, 64 exactly one, 65
# and 257 ragged, 1000 four blocks.
SHAPE_CASES = [
    ("list", 1, 0, 0.1, 2, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1),
    ("list", 2, 1, 0.9, 2, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1),
    ("list", 65, 4, 0.25, 3, (0.25, -0.5, 0.125), (0.5, 0.25, -4.0), 1),
    ("layered", 1, 0, 0.05, 2, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1),
    ("layered", 63, 0, 0.08, 3, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1),
    ("layered", 64, 0, 0.08, 3, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0),
    ("layered", 65, 0, 0.08, 4, (0.0, 0.0, 0.0), (1.0, -2.0, 0.5), 1),
    ("layered", 257, 0, 0.05, 3, (-0.5, 0.25, 1.0), (0.0, 0.0, 0.0), 1),
    ("layered", 1000, 0, 0.04, 5, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0),
    ("layered", 45, 80, 0.07, 6, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1),
]


def case_input(i):
    """(xyz (n, 3), disp (n) or None) of shape case i, read-only"""
    kind, a, b = SHAPE_CASES[i][:3]
    if kind == "list":
        xyz, _ = random_list(a, 900 + b, 0.5)
        xyz.setflags(write=False)
        return xyz, None
    if b:
        xyz, disp, _ = layered_lists(a, b, 700 + a)
        return xyz, disp
    xyz, disp, _ = layered_lists(24, 130, 724)
    ok = np.isfinite(xyz).all(axis=1) & (disp > 0)
    out = np.ascontiguousarray(xyz[ok][:a])
    assert out.shape[0] == a
    out.setflags(write=False)
    return out, None


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
        r, k, o, w, orient = SHAPE_CASES[i][3:]
        xyz, disp = case_input(i)
        return cells(xyz, disp if with_disp else None, r, k, o, w, bool(orient))
    return shared(("case", i, with_disp), make)


def want_of(key, xyz, disp, radius, k, origin=(0.0, 0.0, 0.0), viewpoint=(0.0, 0.0, 0.0), orient=True):
    """the cell form on a named cloud, computed once and shared"""
    return shared((key, float(radius), int(k), tuple(origin), tuple(viewpoint), bool(orient)),
                  lambda: cells(xyz, disp, radius, k, origin, viewpoint, orient))
