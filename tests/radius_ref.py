"""The radius outlier removal of include/sgm_hip_radius.h, restated in numpy, twice: over all pairs (`brute`, in chunks) and over
the 27 cells around each point of the cloud sorted by cell (`cells`, for larger clouds) -- the reference the device results are
held against bit for bit (tests/test_gpu_radius.py), the hand-worked answers of tests/test_radius_reference.py, the case table and
the cloud generators.  Nothing here knows about a hash table, a probe or an arrival order, and every float step is one numpy
float32 operation, rounded to binary32 on its own."""
import numpy as np

import voxel_ref as VR

G_BIAS = 1 << 16
MAX_POINTS = (1 << 24) - 1           # the header's limit on n
FULL = (1 << 24) - 1                 # a max_count no cloud reaches: the full count
F32 = np.float32


def constants(radius):
    """step 2: (r2, v, inv), each one binary32 operation; asserts what the entries refuse"""
    r = F32(radius)
    with np.errstate(all="ignore"):
        r2 = r * r
        v = r * F32(1.03125)
        inv = F32(1.0) / v
    assert np.isfinite(r) and r > 0 and np.isfinite(r2) and r2 >= np.finfo(np.float32).tiny and np.isfinite(inv)
    return r2, v, inv


def classify(xyz, disp, radius, origin):
    """steps 1 and 3: (valid, in_range, g int64 (n, 3)); g means something on in_range rows only"""
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32 and xyz.ndim == 2 and xyz.shape[1] == 3
    _, _, inv = constants(radius)
    o = np.asarray(origin, np.float32).reshape(3)
    assert np.isfinite(o).all()
    valid = np.isfinite(xyz).all(axis=1)
    if disp is not None:
        disp = np.asarray(disp)
        assert disp.dtype == np.float32 and disp.shape == (xyz.shape[0],)
        valid &= disp > 0
    with np.errstate(all="ignore"):
        g = np.floor((xyz - o[None, :]) * inv)           # two float32 operations, then the floor
        inr = valid & ((g >= F32(-G_BIAS)) & (g < F32(G_BIAS))).all(axis=1)
    gi = np.where(inr[:, None], g, F32(0)).astype(np.int64)
    return valid, inr, gi


def d2_of(a, b):
    """step 4 for broadcastable float32 arrays of points (..., 3)"""
    dx, dy, dz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
    out = (dx * dx + dy * dy) + dz * dz
    assert out.dtype == np.float32
    return out


def _finish(xyz, colors, valid, inr, c, nb_points, max_count):
    n = xyz.shape[0]
    keep = (c >= nb_points).astype(np.uint8)
    idx = np.nonzero(keep)[0]
    if colors is not None:
        colors = np.asarray(colors)
        assert colors.dtype == np.uint8 and colors.shape == (n, 3)
    return dict(keep=keep, counts=np.minimum(c, max_count).astype(np.uint32), points=xyz[idx], colors=None if colors is None else colors[idx],
                index=idx.astype(np.uint32), n_kept=int(idx.size), n_out_of_range=int((valid & ~inr).sum()), full=c, in_range=inr)


def brute(xyz, disp=None, colors=None, radius=0.02, nb_points=8, max_count=None, origin=(0.0, 0.0, 0.0), chunk=512):
    """The whole definition over all pairs.  Returns a dict: keep uint8 (n), counts uint32 (n), points, colors, index uint32,
    n_kept, n_out_of_range, and for the tests full int64 (n) -- the unsaturated c_i -- and in_range."""
    xyz = np.asarray(xyz)
    n = xyz.shape[0]
    max_count = nb_points if max_count is None else max_count
    assert n <= MAX_POINTS and 1 <= nb_points <= max_count
    r2, _, _ = constants(radius)
    valid, inr, _ = classify(xyz, disp, radius, origin)
    ids = np.nonzero(inr)[0]
    P = xyz[ids]
    c = np.zeros(n, np.int64)
    for lo in range(0, ids.size, chunk):
        A = P[lo:lo + chunk]
        near = d2_of(A[:, None, :], P[None, :, :]) <= r2
        near[np.arange(A.shape[0]), lo + np.arange(A.shape[0])] = False      # j != i
        c[ids[lo:lo + chunk]] = near.sum(axis=1)
    return _finish(xyz, colors, valid, inr, c, nb_points, max_count)


OFFSETS = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.int64)


def key_of(gi):
    gb = gi + G_BIAS
    return (gb[..., 0] << 34) | (gb[..., 1] << 17) | gb[..., 2]


def cells(xyz, disp=None, colors=None, radius=0.02, nb_points=8, max_count=None, origin=(0.0, 0.0, 0.0), budget=1 << 22):
    """The same through the cells: the points sorted by cell key, and per point the candidates of its 27 neighbour cells (those
    inside the index range), expanded `budget` candidate pairs at a time."""
    xyz = np.asarray(xyz)
    n = xyz.shape[0]
    max_count = nb_points if max_count is None else max_count
    assert n <= MAX_POINTS and 1 <= nb_points <= max_count
    r2, _, _ = constants(radius)
    valid, inr, gi = classify(xyz, disp, radius, origin)
    ids = np.nonzero(inr)[0]
    c = np.zeros(n, np.int64)
    if ids.size:
        key = key_of(gi[ids])
        order = np.argsort(key, kind="stable")
        ids, key, g = ids[order], key[order], gi[ids][order]
        P = xyz[ids]
        m = ids.size
        cs = np.zeros(m, np.int64)
        for off in OFFSETS:
            ng = g + off[None, :]
            ok = ((ng >= -G_BIAS) & (ng < G_BIAS)).all(axis=1)
            nk = key_of(np.where(ok[:, None], ng, 0))
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
                    near = (d2_of(P[i], P[j]) <= r2) & (i != j)
                    cs[a:b] += np.bincount(i[near] - a, minlength=b - a)
                a = b
        c[ids] = cs
    return _finish(xyz, colors, valid, inr, c, nb_points, max_count)


def max_cell_difference(xyz, radius, origin=(0.0, 0.0, 0.0), chunk=512):
    """the lemma of the header, measured over all pairs: the largest |g_a(p) - g_a(q)| among the in-range pairs with d2 <= r2
    (-1 if there is no such pair)"""
    r2, _, _ = constants(radius)
    _, inr, gi = classify(xyz, None, radius, origin)
    P, g = xyz[inr], gi[inr]
    worst = -1
    for lo in range(0, P.shape[0], chunk):
        near = d2_of(P[lo:lo + chunk, None, :], P[None, :, :]) <= r2
        i, j = np.nonzero(near)
        if i.size:
            worst = max(worst, int(np.abs(g[lo + i] - g[j]).max()))
    return worst


# ---- generators ----------------------------------------------------------------------------------------------------------------
def layered_lists(H, W, seed):
    """voxel_ref.layered_cloud as lists (xyz (n, 3), disp (n), colors (n, 3)), read-only"""
    xyz, disp, col = VR.layered_cloud(H, W, seed)
    out = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)
    for a in out:
        a.setflags(write=False)
    return out


def random_list(n, seed, extent=1.0):
    """n points in a cube with clumps, duplicates and a few non-finite rows; colours"""
    rng = np.random.default_rng(seed)
    xyz = (rng.random((n, 3)) * extent - extent / 2).astype(np.float32)
    if n >= 4:
        xyz[n // 2] = xyz[0]                       # a duplicate
        xyz[n // 3, rng.integers(0, 3)] = np.nan   # a hole
    return xyz, rng.integers(0, 256, size=(n, 3), dtype=np.uint8)


def face_pairs(radius, origin=(0.0, 0.0, 0.0), cell=(3, -2, 5)):
    """For each of the 26 directions a pair of points on either side of that face, edge or corner of one cell, well within r of each
    other and far from every other pair: (xyz float32 (52, 3), directions (26, 3)).  Pair k is rows 2k, 2k + 1."""
    _, v, _ = constants(radius)
    o = np.asarray(origin, np.float64)
    dirs = OFFSETS[(OFFSETS != 0).any(axis=1)]
    pts = []
    for k, d in enumerate(dirs):
        base = np.array(cell, np.float64) + np.array([40.0 * (k + 1), 0.0, 0.0])       # a cell of its own per pair
        lo, hi = base * float(v) + o, (base + 1) * float(v) + o
        mid = (lo + hi) / 2
        face = np.where(d > 0, hi, np.where(d < 0, lo, mid))
        eps = 0.2 * float(radius)
        pts.append(face - d * eps)        # inside the cell
        pts.append(face + d * eps)        # across the face, edge or corner: at most 0.4 * sqrt(3) * r away
    return np.array(pts, np.float32), dirs


def lattice(k, spacing, origin=(0.0, 0.0, 0.0)):
    """k^3 points of a cubic lattice (spacing a power of two: all arithmetic exact), and per point on how many of the three axes it
    sits on the boundary"""
    a = np.arange(k)
    g = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=3).reshape(-1, 3)
    on_boundary = ((g == 0) | (g == k - 1)).sum(axis=1)
    return (g.astype(np.float32) * F32(spacing) + np.asarray(origin, np.float32)[None, :]).astype(np.float32), on_boundary


# ---- the case table ------------------------------------------------------------------------------------------------------------
# (kind, a, b, radius, nb_points, max_count, origin).  kind "list": random_list(a, seed 900 + b, extent 0.5); "layered": the
# layered cloud a x b of voxel_ref with seed 700 + its index in voxel_ref's table where it has one.  The kernels work in blocks
# of 256 points and waves of 64: 63 under one wave, 64 exactly one, 65 and 257 ragged.
SHAPE_CASES = [
    ("list", 1, 0, 0.1, 1, 1, (0.0, 0.0, 0.0)),
    ("list", 2, 1, 0.6, 1, 4, (0.0, 0.0, 0.0)),
    ("list", 63, 2, 0.1, 2, 2, (0.0, 0.0, 0.0)),
    ("list", 64, 3, 0.1, 1, FULL, (0.0, 0.0, 0.0)),
    ("list", 65, 4, 0.15, 3, 5, (0.25, -0.5, 0.125)),
    ("list", 257, 5, 0.08, 2, FULL, (0.0, 0.0, 0.0)),
    ("layered", 24, 130, 0.03, 4, 8, (0.0, 0.0, 0.0)),
    ("layered", 48, 320, 0.02, 8, 8, (0.0, 0.0, 0.0)),
    ("layered", 48, 320, 0.02, 16, FULL, (-0.5, 0.25, 1.0)),
    ("layered", 48, 320, 0.01, 4, 6, (0.0, 0.0, 0.0)),
]


def case_input(i):
    kind, a, b = SHAPE_CASES[i][:3]
    if kind == "list":
        xyz, col = random_list(a, 900 + b, 0.5)
        return xyz, None, col
    return layered_lists(a, b, 704 if (a, b) == (48, 320) else 700 + a)


_cache = {}


def case_want(i, with_disp=True):
    """the reference of shape case i (the cell form), computed once and shared (read-only)"""
    k = (i, with_disp)
    if k not in _cache:
        r, nb, mc, o = SHAPE_CASES[i][3:]
        xyz, disp, col = case_input(i)
        res = cells(xyz, disp if with_disp else None, col, r, nb, mc, o)
        for a in res.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[k] = res
    return _cache[k]
