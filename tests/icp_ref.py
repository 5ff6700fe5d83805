"""The rigid registration of include/sgm_hip_icp.h, restated in numpy -- the reference the device results are held against bit for
bit (tests/test_gpu_icp.py), the hand-worked answers of tests/test_icp_reference.py, the case table and the cloud generators.  The
correspondence is stated twice: over all pairs (`correspond_brute`) and over the 27 cells around each transformed source point
(`correspond_cells`, for larger clouds).  Nothing here knows about a hash table, a wave or a launch shape.  Every binary32 step is one
numpy float32 operation, the fused multiply-adds of step 2 are plane_ref's exact emulation; every term is numpy float64 with the
order of the operations written out; the tree is literally a = a[0::2] + a[1::2]; the solve and the update are plain Python floats."""
import math

import numpy as np

import plane_ref as PR
import radius_ref as RR

F32 = np.float32
F64 = np.float64
QNAN = np.uint32(0x7FC00000)
MAX_ITERATION = 1000
STATS = ("valid_source", "target_in_range", "target_out_of_range", "iterations", "correspondences", "unplaced", "unusable_normals",
         "status")
CONVERGED, MAX_ITER, TOO_FEW, DEGENERATE = 0, 1, 2, 3
fmaf = PR.fmaf


def check_T(T):
    """what the entries refuse: (4, 4) float64"""
    T = np.asarray(T, F64).reshape(4, 4)
    assert np.isfinite(T).all() and T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    return T


def m_of(T):
    """step 2: the 12 entries rounded to binary32, (3, 4)"""
    with np.errstate(all="ignore"):
        return np.asarray(T, F64).reshape(4, 4)[:3].astype(F32)


def transform(M, xyz):
    """step 2: p' of every row (also of the rows that are not valid), float32 (n, 3)"""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    cols = [fmaf(M[a, 2], z, fmaf(M[a, 1], y, fmaf(M[a, 0], x, M[a, 3]))) for a in range(3)]
    return np.stack(cols, axis=1).astype(F32).reshape(-1, 3)


def transform_normals(M, nrm):
    """sgm_transform_points on normals: the rotation part, the first term a plain binary32 product"""
    x, y, z = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    with np.errstate(all="ignore"):
        cols = [fmaf(M[a, 2], z, fmaf(M[a, 1], y, M[a, 0] * x)) for a in range(3)]
    return np.stack(cols, axis=1).astype(F32).reshape(-1, 3)


def placed_of(P, valid, r, origin):
    """step 2: which valid source points are placed (p' finite and in range), and the cell of each"""
    fin, inr, g = RR.classify(P, None, r, origin)
    return valid & fin & inr, g


def correspond_brute(P, placed, Q, q_in, r, budget=1 << 22):
    """step 3 over all pairs: (corr int32 (ns), d2 float32 (ns) with QNAN where there is none)"""
    r2, _, _ = RR.constants(r)
    ns = P.shape[0]
    corr = np.full(ns, -1, np.int32)
    d2 = np.full(ns, 0, np.uint32)
    d2[:] = QNAN
    d2 = d2.view(F32)
    tid = np.nonzero(q_in)[0]                     # ascending target index: argmin's first minimum is the lowest index
    sid = np.nonzero(placed)[0]
    if tid.size == 0 or sid.size == 0:
        return corr, d2
    Qi = Q[tid]
    step = max(1, budget // tid.size)
    for lo in range(0, sid.size, step):
        rows = sid[lo:lo + step]
        dd = RR.d2_of(P[rows][:, None, :], Qi[None, :, :])
        k = np.argmin(dd, axis=1)
        best = dd[np.arange(rows.size), k]
        ok = best <= r2
        corr[rows[ok]] = tid[k[ok]]
        d2[rows[ok]] = best[ok]
    return corr, d2


def correspond_cells(P, placed, g, Q, q_in, gq, r, budget=1 << 22):
    """the same through the cells: the in-range target points sorted by cell key, and per placed source point the candidates of the
    27 cells around the cell of p' (those inside the index range)"""
    r2, _, _ = RR.constants(r)
    ns = P.shape[0]
    corr = np.full(ns, -1, np.int32)
    d2 = np.full(ns, 0, np.uint32)
    d2[:] = QNAN
    d2 = d2.view(F32)
    tid = np.nonzero(q_in)[0]
    sid = np.nonzero(placed)[0]
    if tid.size == 0 or sid.size == 0:
        return corr, d2
    key = RR.key_of(gq[tid])
    order = np.argsort(key, kind="stable")
    tid, key = tid[order], key[order]
    Qs = Q[tid]
    best = np.full(sid.size, np.inf, F32)
    bj = np.full(sid.size, np.iinfo(np.int64).max, np.int64)
    gs, Ps = g[sid], P[sid]
    for off in RR.OFFSETS:
        ng = gs + off[None, :]
        ok = ((ng >= -RR.G_BIAS) & (ng < RR.G_BIAS)).all(axis=1)
        nk = RR.key_of(np.where(ok[:, None], ng, 0))
        lo = np.searchsorted(key, nk, side="left")
        ln = np.where(ok, np.searchsorted(key, nk, side="right") - lo, 0)
        ends = np.cumsum(ln)
        a, m = 0, sid.size
        while a < m:
            b = max(a + 1, int(np.searchsorted(ends, (ends[a - 1] if a else 0) + budget, side="right")))
            L = ln[a:b]
            tot = int(L.sum())
            if tot:
                i = np.repeat(np.arange(a, b), L)
                first = np.repeat(np.cumsum(L) - L, L)
                j = np.repeat(lo[a:b], L) + (np.arange(tot) - first)
                dd = RR.d2_of(Ps[i], Qs[j])
                jt = tid[j]
                near = dd <= r2
                i, dd, jt = i[near], dd[near], jt[near]
                if i.size:
                    o = np.lexsort((jt, dd, i))                  # per source point: the smallest d2, then the lowest index
                    i, dd, jt = i[o], dd[o], jt[o]
                    head = np.ones(i.size, bool)
                    head[1:] = i[1:] != i[:-1]
                    i, dd, jt = i[head], dd[head], jt[head]
                    better = (dd < best[i]) | ((dd == best[i]) & (jt < bj[i]))
                    best[i[better]], bj[i[better]] = dd[better], jt[better]
            a = b
    found = np.isfinite(best)
    corr[sid[found]] = bj[found]
    d2[sid[found]] = best[found]
    return corr, d2


def usable_normals(N):
    """step 4: finite, and the binary32 squared length in [0.25, 4]"""
    with np.errstate(all="ignore"):
        len2 = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
        assert len2.dtype == np.float32
        return np.isfinite(N).all(axis=1) & (len2 >= F32(0.25)) & (len2 <= F32(4.0))


def terms(P, Q, N, corr, d2, estimation):
    """step 4: (terms float64 (ns, 28), number of correspondences with an unusable normal)"""
    ns = P.shape[0]
    s = np.zeros((ns, 28), F64)
    has = corr >= 0
    c = corr[has].astype(np.int64)
    p = P[has].astype(F64)
    q = Q[c].astype(F64)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    dx, dy, dz = px - q[:, 0], py - q[:, 1], pz - q[:, 2]
    out = np.zeros((c.size, 28), F64)
    out[:, 27] = d2[has].astype(F64)
    unusable = 0
    if estimation == 1:
        use = usable_normals(N[c])
        unusable = int((~use).sum())
        n = N[c].astype(F64)
        nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
        with np.errstate(all="ignore"):
            e = (nx * dx + ny * dy) + nz * dz
            a = [py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz]
            k = 0
            for r in range(6):
                for t in range(r, 6):
                    out[:, k] = a[r] * a[t]
                    k += 1
            for r in range(6):
                out[:, 21 + r] = -(a[r] * e)
        out[~use, :27] = 0.0
    else:
        one, zero = np.ones(c.size, F64), np.zeros(c.size, F64)
        cols = [py * py + pz * pz, -(px * py), -(px * pz), zero, -pz, py,
                px * px + pz * pz, -(py * pz), pz, zero, -px,
                px * px + py * py, -py, px, zero,
                one, zero, zero, one, zero, one,
                -(py * dz - pz * dy), -(pz * dx - px * dz), -(px * dy - py * dx), -dx, -dy, -dz]
        for k, col in enumerate(cols):
            out[:, k] = col
    s[has] = out
    return s, unusable


def tree(a):
    """step 5 along axis 0: pad with +0.0 to the next power of two, then pairs"""
    a = np.asarray(a, F64)
    n = a.shape[0]
    size = 1
    while size < n:
        size <<= 1
    pad = np.zeros((size - n,) + a.shape[1:], F64)
    a = np.concatenate([a, pad]) if n else np.zeros((1,) + a.shape[1:], F64)
    while a.shape[0] > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def solve(s):
    """step 6 in Python floats: the six unknowns, or None (degenerate)"""
    s = [float(v) for v in s]
    A = [[0.0] * 6 for _ in range(6)]
    k = 0
    for r in range(6):
        for q in range(r, 6):
            A[r][q] = A[q][r] = s[k]
            k += 1
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        v = [L[j][k] * D[k] for k in range(j)]
        dj = A[j][j]
        for k in range(j):
            dj = dj - L[j][k] * v[k]
        if not (math.isfinite(dj) and dj > 0.0):
            return None
        D[j] = dj
        for i in range(j + 1, 6):
            t = A[i][j]
            for k in range(j):
                t = t - L[i][k] * v[k]
            L[i][j] = t / dj
    y = [0.0] * 6
    for i in range(6):
        y[i] = s[21 + i]
        for k in range(i):
            y[i] = y[i] - L[i][k] * y[k]
    for i in range(6):
        y[i] = y[i] / D[i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        x[i] = y[i]
        for k in range(i + 1, 6):
            x[i] = x[i] - L[k][i] * x[k]
    return x if all(math.isfinite(v) for v in x) else None


def rotation_of(x):
    """step 7: the rotation of the quaternion (1, x0 / 2, x1 / 2, x2 / 2), rows of Python floats"""
    qx, qy, qz = x[0] * 0.5, x[1] * 0.5, x[2] * 0.5
    xx, yy, zz = qx * qx, qy * qy, qz * qz
    nn = ((1.0 + xx) + yy) + zz
    return [[(((1.0 + xx) - yy) - zz) / nn, (2.0 * (qx * qy - qz)) / nn, (2.0 * (qx * qz + qy)) / nn],
            [(2.0 * (qx * qy + qz)) / nn, (((1.0 - xx) + yy) - zz) / nn, (2.0 * (qy * qz - qx)) / nn],
            [(2.0 * (qx * qz - qy)) / nn, (2.0 * (qy * qz + qx)) / nn, (((1.0 - xx) - yy) + zz) / nn]]


def update(x, T):
    """step 7: dT * T, float64 (4, 4)"""
    T = [[float(v) for v in row] for row in np.asarray(T, F64).reshape(4, 4)]
    R = rotation_of(x)
    dT = [R[i] + [float(x[3 + i])] for i in range(3)]
    out = [[((dT[i][0] * T[0][j] + dT[i][1] * T[1][j]) + dT[i][2] * T[2][j]) + dT[i][3] * T[3][j] for j in range(4)] for i in range(3)]
    out.append([0.0, 0.0, 0.0, 1.0])
    return np.array(out, F64)


def solve_update(s, T):
    """sgm_icp_solve: (T_out, status)"""
    x = solve(s)
    if x is None:
        return np.asarray(T, F64).reshape(4, 4).copy(), DEGENERATE
    return update(x, T), 0


class Clouds:
    """the two clouds of a call with what does not change from one evaluation to the next"""

    def __init__(self, src, dsrc, tgt, dtgt, nrm, r, origin=(0.0, 0.0, 0.0)):
        self.src = np.asarray(src, F32).reshape(-1, 3)
        self.tgt = np.asarray(tgt, F32).reshape(-1, 3)
        self.nrm = None if nrm is None else np.asarray(nrm, F32).reshape(-1, 3)
        self.r, self.origin = F32(r), origin
        self.valid = PR.valid_of(self.src, None if dsrc is None else np.asarray(dsrc, F32).reshape(-1))
        if self.tgt.shape[0]:
            tv, self.q_in, self.gq = RR.classify(self.tgt, None if dtgt is None else np.asarray(dtgt, F32).reshape(-1), r, origin)
        else:
            RR.constants(r)
            tv = self.q_in = np.zeros(0, bool)
            self.gq = np.zeros((0, 3), np.int64)
        self.m_s = int(self.valid.sum())
        self.t_in, self.t_out = int(self.q_in.sum()), int((tv & ~self.q_in).sum())


def evaluate(cl, T, estimation=0, how="auto", known_corr=None):
    """steps 2 to 5 and the figures of step 8 under T.  how: "brute", "cells" or "auto" (by the number of pairs); known_corr: the
    correspondences where they are known in closed form (their d2 is then computed for those pairs alone)."""
    M = m_of(T)
    P = transform(M, cl.src)
    placed, g = placed_of(P, cl.valid, cl.r, cl.origin)
    if known_corr is not None:
        corr = np.asarray(known_corr, np.int32)
        d2 = np.full(corr.size, 0, np.uint32)
        d2[:] = QNAN
        d2 = d2.view(F32)
        has = corr >= 0
        d2[has] = RR.d2_of(P[has], cl.tgt[corr[has]])
    elif how == "brute" or (how == "auto" and int(placed.sum()) * max(cl.t_in, 1) <= 1 << 24):
        corr, d2 = correspond_brute(P, placed, cl.tgt, cl.q_in, cl.r)
    else:
        corr, d2 = correspond_cells(P, placed, g, cl.tgt, cl.q_in, cl.gq, cl.r)
    s, unusable = terms(P, cl.tgt, cl.nrm, corr, d2, estimation)
    sums = tree(s)
    n_corr = int((corr >= 0).sum())
    fitness = float(n_corr) / float(cl.m_s) if cl.m_s else 0.0
    rmse = math.sqrt(float(sums[27]) / float(n_corr)) if n_corr else 0.0
    return dict(corr=corr, d2=d2, sums=sums, n_corr=n_corr, fitness=fitness, rmse=rmse, unplaced=int((cl.valid & ~placed).sum()),
                unusable=unusable, P=P)


def register(src, dsrc, tgt, dtgt, nrm, r, origin=(0.0, 0.0, 0.0), T0=None, estimation=1, max_iteration=30, rel_fitness=1e-6,
             rel_rmse=1e-6, how="auto"):
    """The whole definition.  Returns T (4, 4), fitness, rmse, corr, d2, history (evaluations, 2), stats uint64 (8) and, for the
    tests, the sums of the last evaluation."""
    T = check_T(np.eye(4) if T0 is None else T0).copy()
    assert estimation in (0, 1) and (estimation == 0 or nrm is not None) and 0 <= max_iteration <= MAX_ITERATION
    assert rel_fitness >= 0 and rel_rmse >= 0
    src = np.asarray(src, F32).reshape(-1, 3)
    if src.shape[0] == 0:
        RR.constants(r)
        return dict(T=T, fitness=0.0, rmse=0.0, corr=np.zeros(0, np.int32), d2=np.zeros(0, F32), history=np.zeros((1, 2), F64),
                    stats=np.array([0, 0, 0, 0, 0, 0, 0, TOO_FEW], np.uint64), sums=np.zeros(28, F64))
    cl = Clouds(src, dsrc, tgt, dtgt, nrm, r, origin)
    ev = evaluate(cl, T, estimation, how)
    hist = [(ev["fitness"], ev["rmse"])]
    it = 0
    while True:
        if ev["n_corr"] < 6:
            status = TOO_FEW
            break
        if it == max_iteration:
            status = MAX_ITER
            break
        x = solve(ev["sums"])
        if x is None:
            status = DEGENERATE
            break
        T = update(x, T)
        prev = ev
        ev = evaluate(cl, T, estimation, how)
        hist.append((ev["fitness"], ev["rmse"]))
        it += 1
        if abs(ev["fitness"] - prev["fitness"]) < rel_fitness and abs(ev["rmse"] - prev["rmse"]) < rel_rmse:
            status = CONVERGED
            break
    stats = np.array([cl.m_s, cl.t_in, cl.t_out, it, ev["n_corr"], ev["unplaced"], ev["unusable"], status], np.uint64)
    return dict(T=T, fitness=ev["fitness"], rmse=ev["rmse"], corr=ev["corr"], d2=ev["d2"], history=np.array(hist, F64), stats=stats,
                sums=ev["sums"])


# ---- generators ----------------------------------------------------------------------------------------------------------------
def corner(n, seed, extent=1.0):
    """n points on the three faces of a corner (the planes x = 0, y = 0, z = 0 over [0, extent]^2, moved off the origin) with their
    unit normals: (xyz float32 (n, 3), normals float32 (n, 3)).  Three planes that meet in a point fix all six unknowns."""
    rng = np.random.default_rng(seed)
    uv = (rng.random((n, 2)) * extent).astype(F32)
    face = np.arange(n) % 3
    xyz = np.zeros((n, 3), F32)
    nrm = np.zeros((n, 3), F32)
    for f in range(3):
        m = face == f
        xyz[m, (f + 1) % 3] = uv[m, 0]
        xyz[m, (f + 2) % 3] = uv[m, 1]
        nrm[m, f] = 1.0
    return (xyz + np.array([0.5, -0.25, 2.0], F32)).astype(F32), nrm


def rigid(axis, degrees, t):
    """a rotation about `axis` by `degrees` and the translation t as float64 (4, 4) (Rodrigues)"""
    a = np.asarray(axis, F64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], F64)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def moved(xyz, nrm, T):
    """the cloud under T in binary64, rounded to float32 once"""
    R, t = T[:3, :3], T[:3, 3]
    p = (xyz.astype(F64) @ R.T + t[None, :]).astype(F32)
    return p, None if nrm is None else (nrm.astype(F64) @ R.T).astype(F32)


R_CASE = 0.1                       # the radius of the generated cases
TRUE_MOTION = rigid((1.0, 2.0, 3.0), 2.0, (0.03, -0.03, 0.025))      # oblique axis; |t| = 0.049, about half of R_CASE


def recovery_case(n=2400, seed=41):
    """a target that is a rigid copy of the source: (src, tgt, target normals, the motion source -> target)"""
    src, nrm = corner(n, seed)
    tgt, tn = moved(src, nrm, TRUE_MOTION)
    return src, tgt, tn, TRUE_MOTION


def pair_case(ns, nt, seed):
    """a generic pair: the target nt points of a corner with normals (every 11th normal zero: unusable; every 13th row NaN), its
    disparities (every 7th not positive); the source ns points of the same corner moved back by a small motion, every 5th far away
    (unplaced), every 6th a few radii off (placed, no partner), every 17th NaN; its disparities (every 9th not positive)"""
    tgt, tn = corner(nt, seed)
    tn = tn.copy()
    tn[np.arange(nt) % 11 == 10] = 0.0
    tgt = tgt.copy()
    tgt[np.arange(nt) % 13 == 12, 1] = np.nan
    dt = np.where(np.arange(nt) % 7 == 6, 0.0, 3.0).astype(F32)
    base, _ = corner(ns, seed + 1000)
    src, _ = moved(base, None, np.linalg.inv(rigid((3.0, 1.0, 2.0), 1.0, (0.01, 0.02, -0.01))))
    i = np.arange(ns)
    src[i % 5 == 4] += F32(1.0e6)
    src[i % 6 == 5] += F32(0.5)
    src[i % 17 == 16, 2] = np.inf
    ds = np.where(i % 9 == 8, -1.0, 2.0).astype(F32)
    out = (np.ascontiguousarray(src), ds, np.ascontiguousarray(tgt), dt, np.ascontiguousarray(tn))
    for a in out:
        a.setflags(write=False)
    return out


# ---- the case table ------------------------------------------------------------------------------------------------------------
# (ns, nt): the kernels work in waves of 64 and blocks of 256 source points (63 under one wave, 64 one, 65 and 257 ragged, 65 537
# more than 256 blocks: the second level of the tree), against a target of one point, of a few cells and of many.
SHAPE_NS = (1, 63, 64, 65, 255, 256, 257, 1000, 65537)
SHAPE_NT = (1, 300, 5000)
SHAPE_CASES = [(ns, nt) for ns in SHAPE_NS for nt in SHAPE_NT]
SHAPE_ITERATIONS = 2

_cache = {}


def shared(key, make):
    """a reference computed once and shared, its arrays read-only"""
    if key not in _cache:
        res = make()
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = res
    return _cache[key]


def case_input(i):
    ns, nt = SHAPE_CASES[i]
    key = ("in", ns, nt)
    if key not in _cache:
        _cache[key] = pair_case(ns, nt, 500 + i)
    return _cache[key]


def case_want(i, with_disp, estimation, how="auto"):
    def make():
        src, ds, tgt, dt, tn = case_input(i)
        return register(src, ds if with_disp else None, tgt, dt if with_disp else None, tn, R_CASE, estimation=estimation,
                        max_iteration=SHAPE_ITERATIONS, how=how)
    return shared(("case", i, with_disp, estimation, how), make)


# ---- the condition cases (tests/test_icp_reference.py asserts the conditions on the reference) ----------------------------------
def condition_case(name):
    """(src, source disparities, tgt, target disparities, target normals, r) of a named case"""
    if name == "layered":          # correspondences, unplaced points and sources without a partner, each a good share
        return pair_case(3000, 3000, 77) + (R_CASE,)
    if name == "tie":              # 300 source points, each exactly between two targets: binary32-equal distances
        k = np.arange(300, dtype=F32)
        src = np.stack([k * F32(4.0), np.zeros(300, F32), np.full(300, 2.0, F32)], axis=1)
        plus, minus = src.copy(), src.copy()
        plus[:, 0] += F32(0.25)
        minus[:, 0] -= F32(0.25)
        first = np.where((np.arange(300) % 2 == 0)[:, None], plus, minus)       # the lower index is the + side for even k
        second = np.where((np.arange(300) % 2 == 0)[:, None], minus, plus)
        tgt = np.ascontiguousarray(np.stack([first, second], axis=1).reshape(-1, 3))
        return np.ascontiguousarray(src), None, tgt, None, None, 0.5
    if name == "plane":            # one plane: point-to-plane cannot fix the motion inside it
        import covariance_ref as CR
        tgt = CR.plane_lattice(12, 16, 0.25, 2.0)
        nrm = np.zeros_like(tgt)
        nrm[:, 2] = 1.0
        src = tgt + np.array([0.03125, 0.0, 0.015625], F32)
        return np.ascontiguousarray(src), None, tgt, None, nrm, 0.125
    if name == "corner":           # three planes: full rank
        src, tgt, tn, _ = recovery_case(900, 43)
        return src, None, tgt, None, tn, R_CASE
    raise KeyError(name)


def big_lattice():
    """more than 1024 blocks of 256 source points with correspondences known in closed form: a 64 x 64 x 65 lattice of spacing 1/4
    against itself shifted by 1/32 along x, r = 1/8: the partner of point i is point i.  (src, tgt, normals, r, corr)"""
    a, b, c = np.meshgrid(np.arange(64), np.arange(64), np.arange(65), indexing="ij")
    src = (np.stack([a, b, c], axis=3).reshape(-1, 3).astype(F32) * F32(0.25)).astype(F32)
    tgt = src + np.array([0.03125, 0.0, 0.0], F32)
    i = np.arange(src.shape[0])
    nrm = np.zeros_like(src)
    nrm[i, i % 3] = 1.0
    return src, np.ascontiguousarray(tgt), nrm, 0.125, i.astype(np.int32)
