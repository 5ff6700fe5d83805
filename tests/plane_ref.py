"""The plane segmentation of include/sgm_hip_plane.h, restated in numpy -- the reference the device results are held against bit
for bit (tests/test_gpu_plane.py), the hand-worked answers of tests/test_plane_reference.py and the case table.  Nothing here knows
about a tile, a chunk, a matrix core or an arrival order.  Every binary32 step is one numpy float32 operation, every binary64 step
one numpy float64 operation; the fused multiply-add of step 5 is emulated exactly (`fmaf`); the nine sums are np.int64; the 3 x 3
problem is covariance_ref._solve, imported, not copied."""
import numpy as np

import covariance_ref as CR
import radius_ref as RR

F32 = np.float32
F64 = np.float64
QNAN = np.uint32(0x7FC00000)
MAX_K = 65536
REFIT_RANGE = F32(524288.0)
STATS = ("valid", "degenerate", "best", "best_count", "refit_points", "out_of_refit_range", "refined", "found")


def fmaf(a, b, c):
    """fma(a, b, c) in binary32, exactly, elementwise: the product of two binary32 numbers is exact in binary64; the sum with c is
    formed by an error-free TwoSum; where the error term is not zero and the sum's last mantissa bit is even the sum moves one ulp
    towards the error (round to odd); the rounding to binary32 of that is the correctly rounded fused result (53 >= 2 * 24 + 2).
    Operands or sums that are not finite take the plain binary64 expression, which has the right infinity or NaN."""
    a, b, c = (np.asarray(v, F32).astype(F64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        up = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        return np.where(fix, up, s).astype(F32)


def distance(model, xyz):
    """step 5: s = fmaf(c, z, fmaf(b, y, fmaf(a, x, d))) for the plane(s) model (..., 4) and the points xyz (n, 3), broadcast"""
    model = np.asarray(model, F32)
    a, b, c, d = (model[..., i] for i in range(4))
    return fmaf(c, xyz[..., 2], fmaf(b, xyz[..., 1], fmaf(a, xyz[..., 0], d)))


def is_inlier(s, t):
    with np.errstate(all="ignore"):
        return np.abs(s) <= F32(t)


def hash32(seed, c):
    """step 3: the hash of counter(s) c, uint32 arithmetic mod 2^32 (held in uint64)"""
    M = np.uint64(0xFFFFFFFF)
    x = (np.uint64(seed) ^ ((np.asarray(c, np.uint64) * np.uint64(0x9E3779B9)) & M)) & M
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M
    x ^= x >> np.uint64(16)
    return x


def ranks(seed, K, m):
    """step 3: the sample ranks (K, 3) among m valid points"""
    c = np.arange(3 * K, dtype=np.uint64).reshape(K, 3)
    return ((hash32(seed, c) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def qscale_of(t):
    """step 2"""
    t = F32(t)
    assert np.isfinite(t) and t > 0 and t >= np.finfo(np.float32).tiny
    with np.errstate(all="ignore"):
        qs = F32(32.0) / t
    assert np.isfinite(qs)
    return qs


def valid_of(xyz, disp):
    """step 1"""
    v = np.isfinite(xyz).all(axis=1)
    if disp is not None:
        with np.errstate(all="ignore"):
            v &= np.asarray(disp) > 0
    return v


def orient_round(a, b, c, d):
    """step 9 on binary64 values (arrays or scalars): float32 (..., 4)"""
    a, b, c, d = (np.asarray(v, F64) for v in (a, b, c, d))
    first = np.where(a != 0, a, np.where(b != 0, b, c))
    neg = (d < 0) | ((d == 0) & (first < 0))
    sgn = np.where(neg, -1.0, 1.0)
    with np.errstate(all="ignore"):
        out = np.stack([(sgn * v).astype(F32) for v in (a, b, c, d)], axis=-1)      # (a sign change is exact)
        return out + F32(0.0)


def hypotheses(P, rk):
    """step 4 for the valid points P (m, 3) float32 and the ranks rk (K, 3): (planes float32 (K, 4), degenerate bool (K)); the
    plane of a degenerate hypothesis is NaN"""
    p0, p1, p2 = (P[rk[:, j]].astype(F64) for j in range(3))
    with np.errstate(all="ignore"):
        e1, e2 = p1 - p0, p2 - p0
        n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        len2 = (n0 * n0 + n1 * n1) + n2 * n2
        deg = ~(np.isfinite(len2) & (len2 > 0))
        ln = np.sqrt(len2)
        n0, n1, n2 = n0 / ln, n1 / ln, n2 / ln
        d = -((n0 * p0[:, 0] + n1 * p0[:, 1]) + n2 * p0[:, 2])
        planes = orient_round(n0, n1, n2, d)
    planes[deg] = np.nan
    return planes, deg


def counts_of(planes, P, t, budget=1 << 22):
    """step 5: cnt_k over all valid points, `budget` pairs at a time"""
    K, m = planes.shape[0], P.shape[0]
    cnt = np.zeros(K, np.int64)
    step = max(1, budget // max(m, 1))
    for lo in range(0, K, step):
        s = distance(planes[lo:lo + step, None, :], P[None, :, :])
        cnt[lo:lo + step] = is_inlier(s, t).sum(axis=1)
    return cnt


def moments(P, inl, anchor, qs):
    """step 7: (S int64 (9), m_r, inliers out of refit range) over the inliers `inl` of the valid points P"""
    with np.errstate(all="ignore"):
        u = (P[inl] - anchor[None, :]) * qs
        inr = (np.abs(u) <= REFIT_RANGE).all(axis=1)
    assert u.dtype == np.float32
    q = np.rint(u[inr]).astype(np.int64)
    S = [int(q[:, a].sum()) for a in range(3)] + [int((q[:, a] * q[:, b]).sum()) for a, b in CR.PAIRS]
    return S, int(inr.sum()), int((~inr).sum())


def refit(S, m_r, anchor, qs):
    """step 7 from the sums: the refitted plane float32 (4), or None where the model stays the hypothesis'"""
    if m_r < 3:
        return None
    got = CR._solve(tuple(S), int(m_r))
    if got is None:
        return None
    (n0, n1, n2), _, _ = got
    g = [float(anchor[a]) + (float(S[a]) / float(m_r)) / float(qs) for a in range(3)]
    d = -((n0 * g[0] + n1 * g[1]) + n2 * g[2])
    return orient_round(n0, n1, n2, d)


def classify(xyz, disp, colors, model, t, select, found=True):
    """step 8 with the final model"""
    n = xyz.shape[0]
    valid = valid_of(xyz, disp)
    dist = np.full(n, np.nan, np.float32).view(np.uint32)
    dist[:] = QNAN
    dist = dist.view(np.float32)
    inl = np.zeros(n, bool)
    if found:
        dist[valid] = distance(model, xyz[valid])
        inl[valid] = is_inlier(dist[valid], t)
    sel = (valid & ~inl) if select else inl
    idx = np.nonzero(sel)[0].astype(np.uint32)
    return dict(inlier=inl.astype(np.uint8), distance=dist, n_inliers=int(inl.sum()), n_selected=int(sel.sum()), index=idx,
                points=xyz[sel], colors=None if colors is None else colors[sel], selected=sel.astype(np.uint8))


def segment(xyz, disp=None, colors=None, t=0.03, K=64, seed=0, refine=True, select=0):
    """The whole definition.  Returns the outputs of the header (model, inlier, distance, points, colors, index, n_inliers,
    n_selected, stats) and for the tests counts (K), planes (K, 4), degenerate (K), ranks (K, 3) and selected (n)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    disp = None if disp is None else np.asarray(disp, np.float32).reshape(-1)
    colors = None if colors is None else np.asarray(colors).reshape(-1, 3)
    assert 1 <= K <= MAX_K and xyz.shape[0] <= RR.MAX_POINTS and 0 <= seed < 2 ** 32
    qs = qscale_of(t)
    valid = valid_of(xyz, disp)
    P = xyz[valid]
    m = P.shape[0]
    model = np.zeros(4, np.float32)
    stats = np.zeros(8, np.uint64)
    stats[0] = m
    extra = dict(counts=np.zeros(K, np.int64), planes=np.full((K, 4), np.nan, np.float32), degenerate=np.zeros(K, bool),
                 ranks=np.zeros((K, 3), np.int64))
    found = False
    if m >= 3:
        rk = ranks(seed, K, m)
        planes, deg = hypotheses(P, rk)
        cnt = counts_of(planes, P, t)
        assert not cnt[deg].any()
        kb = int(np.argmax(cnt))                      # the first of the largest
        cb = int(cnt[kb])
        found = cb >= 3
        stats[1:4] = int(deg.sum()), kb, cb
        extra = dict(counts=cnt, planes=planes, degenerate=deg, ranks=rk)
        if found:
            model = planes[kb].copy()
            if refine:
                anchor = P[rk[kb, 0]]
                inl = is_inlier(distance(model, P), t)
                S, m_r, oor = moments(P, inl, anchor, qs)
                better = refit(S, m_r, anchor, qs)
                stats[4:6] = m_r, oor
                extra["moments"] = S
                if better is not None:
                    model = better
                    stats[6] = 1
            stats[7] = 1
    out = classify(xyz, disp, colors, model, t, select, found)
    out.update(model=model, stats=stats, **extra)
    return out


def lifted_lattice(H, W, spacing=0.25, z=2.0, every=7, lift=0.5):
    """covariance_ref.plane_lattice with every `every`-th point lifted by `lift`: (xyz (H * W, 3), lifted bool)"""
    xyz = CR.plane_lattice(H, W, spacing, z)
    up = np.arange(H * W) % every == every - 1
    xyz[up, 2] += F32(lift)
    return xyz, up


# ---- the case table ------------------------------------------------------------------------------------------------------------
# (kind, a, b, t, K, seed, refine, select).  kind "list": the first a valid points of the 24 x 130 layered cloud (seed 724) as a
# list; "layered": the a x b layered cloud of voxel_ref (seed 700 + a) with its disparities and colours.  The kernels work in
# waves of 64 points or hypotheses, tiles of 16 x 16, chunks of 1024 points and tiles of 64 hypotheses.
SHAPE_CASES = [("list", n, 0, 0.05, 16, 3, 1, 0) for n in (1, 2, 3, 4, 63, 64, 65, 257, 4097)]
SHAPE_CASES += [("list", 257, 0, 0.05, K, 5, 1, 0) for K in (1, 15, 16, 17, 63, 64, 65, 257, 1000, 4097)]
SHAPE_CASES += [("layered", 24, 130, t, 64, 7, r, s) for t in (0.03, 0.008) for r in (0, 1) for s in (0, 1)]
SHAPE_CASES += [("layered", 48, 320, t, 64, 7, r, s) for t, r, s in ((0.03, 1, 0), (0.03, 0, 1), (0.008, 1, 1), (0.008, 0, 0))]

_cache = {}


def case_input(i):
    """(xyz (n, 3), disp (n) or None, colors (n, 3) or None) of shape case i, read-only"""
    kind, a, b = SHAPE_CASES[i][:3]
    if kind == "layered":
        return RR.layered_lists(a, b, 700 + a)
    key = ("pool",)
    if key not in _cache:
        pool = []
        for s in (724, 725, 726):
            xyz, disp, _ = RR.layered_lists(24, 130, s)
            pool.append(xyz[valid_of(xyz, disp)])
        _cache[key] = np.ascontiguousarray(np.concatenate(pool))
    out = np.ascontiguousarray(_cache[key][:a])
    assert out.shape[0] == a
    out.setflags(write=False)
    return out, None, None


def shared(key, make):
    """a reference computed once and shared, its arrays read-only"""
    if key not in _cache:
        res = make()
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = res
    return _cache[key]


def case_want(i, with_disp=True, with_colors=True):
    def make():
        t, K, seed, refine, select = SHAPE_CASES[i][3:]
        xyz, disp, col = case_input(i)
        return segment(xyz, disp if with_disp else None, col if with_colors else None, t, K, seed, bool(refine), select)
    return shared(("case", i, with_disp, with_colors), make)


def want_of(key, xyz, disp, colors, t, K, seed, refine=True, select=0):
    """the reference on a named cloud, computed once and shared"""
    return shared((key, float(t), K, seed, bool(refine), select, disp is None, colors is None),
                  lambda: segment(xyz, disp, colors, t, K, seed, refine, select))


# ---- the four condition cases of the issue (tests/test_plane_reference.py asserts the conditions on the reference) ---------------
def condition_case(name):
    """(xyz, disp, colors, t, K, seed) of a named case"""
    if name == "layered":          # (i) the best count between 0.2 and 0.6 of the valid points, refined
        xyz, disp, col = RR.layered_lists(48, 320, 704)
        return xyz, disp, col, 0.03, 64, 7
    if name == "tie":              # (ii) two parallel lattices of equal size: hypotheses on different planes hold the maximum
        a = CR.plane_lattice(12, 16, 0.25, 2.0)
        b = CR.plane_lattice(12, 16, 0.25, 3.0)
        return np.ascontiguousarray(np.concatenate([a, b])), None, None, 0.01, 64, 11
    if name == "duplicates":       # (iii) few distinct points: many hypotheses draw a point twice
        base = CR.plane_lattice(2, 3, 0.25, 2.0)
        xyz = np.ascontiguousarray(np.tile(base, (40, 1)))
        return xyz, None, None, 0.01, 64, 13
    if name == "refit_range":      # (iv) a long thin strip in the plane: inliers on both sides of +-16384 t
        t = 0.001
        k = np.arange(400, dtype=np.float32)
        xyz = np.stack([k * F32(0.125) - F32(1.0), (k % 5) * F32(0.25), np.full(400, 2.0, np.float32)], axis=1).astype(np.float32)
        return np.ascontiguousarray(xyz), None, None, t, 64, 17
    raise KeyError(name)
