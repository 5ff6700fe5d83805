"""The density clustering of include/sgm_hip_dbscan.h, restated in numpy, twice: over all pairs (`brute`: a dense matrix of d2, a
breadth-first search over the core points, and per border point a sort of its core neighbours) and over the 27 cells around each
point of the cloud sorted by cell (`cells`, for larger clouds: the linked pairs as lists, the components by propagating the
smallest index, the nearest core point by a minimum over 64-bit keys) -- the reference the device results are held against bit for
bit (tests/test_gpu_dbscan.py), the hand-worked answers of tests/test_dbscan_reference.py, the case table and the generators.
Steps 1 to 5 -- validity, range, distance, the count and with it the core mask -- are tests/radius_ref.py's.  Nothing here knows
about a hash table, a union-find forest on the device or an arrival order."""
import numpy as np

import radius_ref as RR

F32 = np.float32
FULL = RR.FULL
MAX_POINTS = RR.MAX_POINTS
STATS = ("in_range", "out_of_range", "core", "border", "noise", "clusters")
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _finish(n, valid, inr, core, root, nearest):
    """steps 8 to 10 from: core bool (n); root int64 (n), on core points the smallest core index of the point's component;
    nearest int64 (n), on the other points the nearest core point or -1"""
    owner = np.where(core, np.arange(n), nearest)                        # the core point a point hangs on, or -1
    has = owner >= 0
    rep = np.where(has, root[np.where(has, owner, 0)], -1)               # step 9: the representative of its cluster
    reps = np.unique(rep[has])                                           # ascending: the clusters in the order of their numbers
    labels = np.where(has, np.searchsorted(reps, rep), -1).astype(np.int32)
    sizes = np.bincount(labels[has], minlength=reps.size).astype(np.uint32)
    border = inr & ~core & has
    noise = inr & ~has
    stats = np.array([inr.sum(), (valid & ~inr).sum(), core.sum(), border.sum(), noise.sum(), reps.size], np.uint64)
    return dict(labels=labels, core=core.astype(np.uint8), sizes=sizes, n_clusters=int(reps.size), stats=stats, in_range=inr,
                border=border, noise=noise, representatives=reps)


def brute(xyz, disp=None, eps=0.02, min_points=4, origin=(0.0, 0.0, 0.0)):
    """The whole definition over all pairs (a dense matrix: a few thousand points at the most)."""
    xyz = np.asarray(xyz)
    n = xyz.shape[0]
    assert n <= 6000 and 1 <= min_points <= MAX_POINTS
    r2, _, _ = RR.constants(eps)
    first = RR.brute(xyz, disp, None, eps, min_points, FULL, origin)     # steps 1 to 5
    valid, inr, _ = RR.classify(xyz, disp, eps, origin)
    core = first["full"] >= min_points
    assert np.array_equal(core, first["keep"].astype(bool)) and not (core & ~inr).any()
    ids = np.nonzero(inr)[0]
    P = xyz[ids]
    m = ids.size
    D = np.zeros((m, m), np.float32)
    for lo in range(0, m, 512):
        D[lo:lo + 512] = RR.d2_of(P[lo:lo + 512, None, :], P[None, :, :])
    near = D <= r2
    near[np.arange(m), np.arange(m)] = False
    c = core[ids]
    root = np.full(n, -1, np.int64)
    for s in range(m):                                                   # step 6: breadth first from each core point not yet seen,
        if not c[s] or root[ids[s]] >= 0:                                # in ascending source index, so s is its component's smallest
            continue
        root[ids[s]] = ids[s]
        queue = [s]
        while queue:
            a = queue.pop()
            for b in np.nonzero(near[a] & c)[0]:
                if root[ids[b]] < 0:
                    root[ids[b]] = ids[s]
                    queue.append(b)
    nearest = np.full(n, -1, np.int64)
    for a in np.nonzero(~c)[0]:                                          # step 7: the smallest d2 as binary32, then the smallest index
        cand = np.nonzero(near[a] & c)[0]
        if cand.size:
            order = np.lexsort((ids[cand], D[a, cand].view(np.uint32)))   # (d2 >= 0: its bits order as its value)
            assert (np.diff(D[a, cand][order]) >= 0).all()
            nearest[ids[a]] = ids[cand[order[0]]]
    return _finish(n, valid, inr, core, root, nearest)


def linked_pairs(xyz, inr, gi, r2, budget=1 << 22):
    """every ordered pair (i, j), i != j, of in-range points with d2 <= r2, found through the 27 cells: (i, j, d2), source indices"""
    ids = np.nonzero(inr)[0]
    out_i, out_j, out_d = [], [], []
    if ids.size:
        key = RR.key_of(gi[ids])
        order = np.argsort(key, kind="stable")
        ids, key, g = ids[order], key[order], gi[ids][order]
        P = xyz[ids]
        m = ids.size
        for off in RR.OFFSETS:
            ng = g + off[None, :]
            ok = ((ng >= -RR.G_BIAS) & (ng < RR.G_BIAS)).all(axis=1)
            nk = RR.key_of(np.where(ok[:, None], ng, 0))
            lo = np.searchsorted(key, nk, side="left")
            ln = np.where(ok, np.searchsorted(key, nk, side="right") - lo, 0)
            ends = np.cumsum(ln)
            a = 0
            while a < m:
                b = max(a + 1, int(np.searchsorted(ends, (ends[a - 1] if a else 0) + budget, side="right")))
                L = ln[a:b]
                tot = int(L.sum())
                if tot:
                    i = np.repeat(np.arange(a, b), L)
                    first = np.repeat(np.cumsum(L) - L, L)
                    j = np.repeat(lo[a:b], L) + (np.arange(tot) - first)
                    d2 = RR.d2_of(P[i], P[j])
                    hit = (d2 <= r2) & (i != j)
                    out_i.append(ids[i[hit]])
                    out_j.append(ids[j[hit]])
                    out_d.append(d2[hit])
                a = b
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return cat(out_i, np.int64), cat(out_j, np.int64), cat(out_d, np.float32)


def cells(xyz, disp=None, eps=0.02, min_points=4, origin=(0.0, 0.0, 0.0)):
    """The same through the cells and without a search: the components by propagating the smallest index along the links."""
    xyz = np.asarray(xyz)
    n = xyz.shape[0]
    assert n <= MAX_POINTS and 1 <= min_points <= MAX_POINTS
    r2, _, _ = RR.constants(eps)
    valid, inr, gi = RR.classify(xyz, disp, eps, origin)
    i, j, d2 = linked_pairs(xyz, inr, gi, r2)
    core = np.bincount(i, minlength=n) >= min_points                     # step 5
    both = core[i] & core[j]
    ei, ej = i[both], j[both]                                            # step 6 (each link in both directions)
    root = np.arange(n, dtype=np.int64)
    while True:
        new = root.copy()
        np.minimum.at(new, ei, root[ej])
        while True:                                                      # follow the pointers to their ends
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, root):
            break
        root = new
    root = np.where(core, root, -1)
    to_core = ~core[i] & core[j]                                         # step 7
    best = np.full(n, NONE, np.uint64)
    np.minimum.at(best, i[to_core], d2[to_core].view(np.uint32).astype(np.uint64) << np.uint64(32) | j[to_core].astype(np.uint64))
    nearest = np.where(best == NONE, -1, (best & np.uint64(0xFFFFFFFF)).astype(np.int64))
    return _finish(n, valid, inr, core, root, nearest)


def partition(res):
    """what does not depend on the numbering: the clusters as a sorted list of sorted index tuples"""
    lab = res["labels"]
    return sorted(tuple(np.nonzero(lab == c)[0].tolist()) for c in range(res["n_clusters"]))


# ---- generators ----------------------------------------------------------------------------------------------------------------
def chain(count, eps, step=0.9, start=(0.0, 0.0, 0.0), sign=1.0):
    """count points spaced step * eps along the diagonal sign * (1, 1, 1) / sqrt(3), from start"""
    t = np.arange(count, dtype=np.float64) * (sign * step * float(eps)) / np.sqrt(3.0)
    return (np.asarray(start, np.float64)[None, :] + t[:, None]).astype(np.float32)


def beyond(p, direction, eps):
    """the first point on the ray from p along direction (+-1 on one axis) that is not within eps of p: one ulp nearer it still is"""
    r2, _, _ = RR.constants(eps)
    p = np.asarray(p, np.float32)
    d = np.asarray(direction, np.float32)
    away = np.where(d > 0, F32(np.inf), F32(-np.inf))
    q = (p + d * F32(0.999) * F32(eps)).astype(np.float32)
    assert RR.d2_of(p, q) <= r2
    while RR.d2_of(p, q) <= r2:
        q = np.where(d != 0, np.nextafter(q, away), q).astype(np.float32)
    back = np.where(d != 0, np.nextafter(q, p), q).astype(np.float32)
    assert RR.d2_of(p, back) <= r2 < RR.d2_of(p, q)
    return q


def two_chains(count, eps):
    """two chains of count points each: the first from the origin along +(1, 1, 1), the second from a point one ulp beyond eps of
    the origin on the -x axis along -(1, 1, 1).  The two first points are the closest pair of the two chains, every other pair
    being farther by the steps both have taken away from each other."""
    a = chain(count, eps)
    q = beyond(a[0], (-1, 0, 0), eps)
    return a, chain(count, eps, start=q, sign=-1.0)


def stripes(rows, cols, spacing, every):
    """a rows x cols lattice in the plane z = 2 with every `every`-th row (every - 1, 2 * every - 1, ...) removed"""
    y, x = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    keep = (y % every) != every - 1
    pts = np.stack([x * spacing, y * spacing, np.full(x.shape, 2.0)], axis=2).astype(np.float32)
    return pts[keep], keep


def layered_lists(H, W, seed):
    return RR.layered_lists(H, W, seed)[:2]


# ---- the case table ------------------------------------------------------------------------------------------------------------
# (kind, a, b, eps, min_points, origin).  kind "list": radius_ref.random_list(a, seed 900 + b, extent 0.5); "layered": the layered
# cloud a x b of voxel_ref.  63 under one wave, 64 exactly one, 65 and 257 ragged, 4097 more than sixteen blocks.  The layered rows
# are chosen so that the reference finds at least 3 clusters and core, border and noise points are each at least 5 % of the points
# in range (tests/test_dbscan_reference.py asserts it).
SHAPE_CASES = [
    ("list", 1, 0, 0.1, 1, (0.0, 0.0, 0.0)),
    ("list", 2, 1, 0.6, 1, (0.0, 0.0, 0.0)),
    ("list", 63, 2, 0.1, 2, (0.0, 0.0, 0.0)),
    ("list", 64, 3, 0.1, 1, (0.0, 0.0, 0.0)),
    ("list", 65, 4, 0.15, 3, (0.25, -0.5, 0.125)),
    ("list", 257, 5, 0.08, 2, (0.0, 0.0, 0.0)),
    ("list", 4097, 6, 0.03, 3, (0.0, 0.0, 0.0)),
    ("layered", 24, 130, 0.05, 8, (0.0, 0.0, 0.0)),
    ("layered", 48, 320, 0.02, 8, (0.0, 0.0, 0.0)),
    ("layered", 48, 320, 0.02, 6, (-0.5, 0.25, 1.0)),
    ("layered", 48, 320, 0.01, 4, (0.0, 0.0, 0.0)),
]
LAYERED_ROWS = [i for i, c in enumerate(SHAPE_CASES) if c[0] == "layered"]


def case_input(i):
    kind, a, b = SHAPE_CASES[i][:3]
    if kind == "list":
        return RR.random_list(a, 900 + b, 0.5)[0], None
    return layered_lists(a, b, 704 if (a, b) == (48, 320) else 700 + a)


_cache = {}


def case_want(i, with_disp=True):
    """the reference of shape case i (the cell form), computed once and shared (read-only)"""
    k = (i, with_disp)
    if k not in _cache:
        eps, mp, o = SHAPE_CASES[i][3:]
        xyz, disp = case_input(i)
        _cache[k] = freeze(cells(xyz, disp if with_disp else None, eps, mp, o))
    return _cache[k]


def freeze(res):
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


def want_of(name, xyz, disp, eps, min_points, origin=(0.0, 0.0, 0.0)):
    """a shared reference under a name of the caller's"""
    k = (name, float(eps), int(min_points), tuple(float(x) for x in origin), disp is None)
    if k not in _cache:
        _cache[k] = freeze(cells(xyz, disp, eps, min_points, origin))
    return _cache[k]
