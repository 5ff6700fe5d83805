"""The voxel-grid downsampling of include/sgm_hip_voxel.h, restated in numpy: the reference the device results are held against bit
for bit (tests/test_gpu_voxel.py), the hand-worked answers of tests/test_voxel_reference.py, the cloud generator and the shape
list.  Voxels are grouped with np.unique over the 63-bit keys and summed with np.add.at in int64 -- nothing here knows about a hash
table, a probe or an arrival order -- and every float step is one numpy float32 operation, rounded to binary32 on its own."""
import numpy as np

G_BIAS = 1 << 20
MAX_POINTS = (1 << 24) - 1           # the header's limit on n
F32 = np.float32


def classify(xyz, disp, voxel_size, origin):
    """steps 1 and 2: (valid, in_range, g float32 (n, 3), u int64 (n, 3)); g and u mean something on in_range rows only"""
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32 and xyz.ndim == 2 and xyz.shape[1] == 3
    v = F32(voxel_size)
    inv = F32(1.0) / v                                   # binary32, once
    o = np.asarray(origin, np.float32).reshape(3)
    assert np.isfinite(v) and v > 0 and np.isfinite(inv) and np.isfinite(o).all()
    valid = np.isfinite(xyz).all(axis=1)
    if disp is not None:
        disp = np.asarray(disp)
        assert disp.dtype == np.float32 and disp.shape == (xyz.shape[0],)
        valid &= disp > 0
    with np.errstate(all="ignore"):
        t = (xyz - o[None, :]) * inv                     # two float32 operations
        g = np.floor(t)
        inr = valid & ((g >= F32(-G_BIAS)) & (g < F32(G_BIAS))).all(axis=1)
        f = t - g
        u = np.where(inr[:, None], f * F32(65536.0), F32(0)).astype(np.int64)
    u = np.minimum(u, 65535)
    assert (u[inr] >= 0).all()
    return valid, inr, g, u


def keys_of(g):
    gi = g.astype(np.int64) + G_BIAS
    return (gi[:, 0] << 42) | (gi[:, 1] << 21) | gi[:, 2]


def voxel_downsample(xyz, disp=None, colors=None, voxel_size=0.05, origin=(0.0, 0.0, 0.0), min_points=1):
    """The whole definition.  Returns a dict: points float32 (M, 3), colors uint8 (M, 3) or None, counts uint32 (M), n_voxels,
    n_out_of_range, and for the tests keys int64 (M), first int64 (M)."""
    xyz = np.asarray(xyz)
    n = xyz.shape[0]
    assert n <= MAX_POINTS and min_points >= 1
    v = F32(voxel_size)
    o = np.asarray(origin, np.float32).reshape(3)
    valid, inr, g, u = classify(xyz, disp, voxel_size, origin)
    n_oor = int((valid & ~inr).sum())
    idx = np.nonzero(inr)[0]
    if colors is not None:
        colors = np.asarray(colors)
        assert colors.dtype == np.uint8 and colors.shape == (n, 3)
    if idx.size == 0:
        return dict(points=np.zeros((0, 3), np.float32), colors=None if colors is None else np.zeros((0, 3), np.uint8),
                    counts=np.zeros(0, np.uint32), n_voxels=0, n_out_of_range=n_oor, keys=np.zeros(0, np.int64),
                    first=np.zeros(0, np.int64))
    key = keys_of(g[idx])
    uniq, inverse = np.unique(key, return_inverse=True)
    inverse = inverse.reshape(-1)
    nv = uniq.size
    c = np.bincount(inverse, minlength=nv).astype(np.int64)
    S = np.zeros((nv, 3), np.int64)
    np.add.at(S, inverse, u[idx])
    first = np.full(nv, n, np.int64)
    np.minimum.at(first, inverse, idx)
    keep = np.nonzero(c >= min_points)[0]
    keep = keep[np.argsort(first[keep], kind="stable")]          # (first is unique per voxel)
    c, S, first, uniq = c[keep], S[keep], first[keep], uniq[keep]
    M = (2 * S + c[:, None]) // (2 * c[:, None])
    assert M.min(initial=0) >= 0 and M.max(initial=0) <= 65535
    m = M.astype(np.float32) * F32(1.0 / 65536.0)               # exact
    gk = np.stack([(uniq >> 42) & 0x1FFFFF, (uniq >> 21) & 0x1FFFFF, uniq & 0x1FFFFF], axis=1) - G_BIAS
    pts = (gk.astype(np.float32) + m) * v + o[None, :]          # three float32 operations in this order
    assert pts.dtype == np.float32
    col = None
    if colors is not None:
        C = np.zeros((nv, 3), np.int64)
        np.add.at(C, inverse, colors[idx].astype(np.int64))
        C = C[keep]
        col = ((2 * C + c[:, None]) // (2 * c[:, None])).astype(np.uint8)
    return dict(points=pts, colors=col, counts=c.astype(np.uint32), n_voxels=int(keep.size), n_out_of_range=n_oor, keys=uniq,
                first=first)


def layered_cloud(H, W, seed, holes=0.08, nonpositive=0.04):
    """An organised cloud the way a reprojection leaves it: depth in three layers of blocks with noise, X and Y from the pixel
    grid, NaN / inf holes in any of the three coordinates, a float32 disparity that is <= 0 on some pixels, random colours.
    Returns (xyz float32 (H, W, 3), disp float32 (H, W), colors uint8 (H, W, 3)); extents of about 2 x 1 x 3 units."""
    rng = np.random.default_rng(seed)
    fpx = 0.9 * max(W, 8)
    bh, bw = (16, 40) if H > 8 else (1, 16)
    lev = rng.choice(np.array([1.2, 2.0, 3.1]), size=((H + bh - 1) // bh, (W + bw - 1) // bw))
    Z = np.kron(lev, np.ones((bh, bw)))[:H, :W] + rng.normal(0, 0.01, size=(H, W))
    y, x = np.mgrid[0:H, 0:W]
    X = (x - W / 2 + 0.5) * Z / fpx
    Y = (y - H / 2 + 0.5) * Z / fpx
    xyz = np.stack([X, Y, Z], axis=2).astype(np.float32)
    disp = (fpx * 0.1 / Z).astype(np.float32)
    bad = rng.random((H, W)) < holes
    axis = rng.integers(0, 3, size=(H, W))
    what = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=(H, W))
    for a in range(3):
        sel = bad & (axis == a)
        xyz[sel, a] = what[sel]
    neg = rng.random((H, W)) < nonpositive
    disp[neg] = np.where(rng.random(int(neg.sum())) < 0.5, 0.0, -1.0).astype(np.float32)
    colors = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return xyz, disp, colors


# (H, W, voxel_size, origin, min_points): the shapes of the issue.  The kernels work in blocks of 256 points and waves of 64:
#   1 x 63 under one wave, 1 x 64 exactly one, 3 x 257 ragged past a block, the other two many blocks with a ragged last one
SHAPE_CASES = [
    (1, 1, 0.05, (0.0, 0.0, 0.0), 1),
    (1, 63, 0.05, (0.0, 0.0, 0.0), 1),
    (1, 64, 0.02, (0.0, 0.0, 0.0), 1),
    (3, 257, 0.05, (0.0, 0.0, 0.0), 1),
    (48, 320, 0.05, (0.0, 0.0, 0.0), 1),
    (97, 331, 0.03, (-0.5, 0.25, 1.0), 2),
]


def case_input(i):
    H, W = SHAPE_CASES[i][:2]
    return layered_cloud(H, W, 700 + i)


_cache = {}


def case_want(i, with_disp=True, with_colors=True):
    """the reference of shape case i, computed once and shared (read-only)"""
    k = (i, with_disp, with_colors)
    if k not in _cache:
        H, W, v, o, mp = SHAPE_CASES[i]
        xyz, disp, col = case_input(i)
        r = voxel_downsample(xyz.reshape(-1, 3), disp.reshape(-1) if with_disp else None, col.reshape(-1, 3) if with_colors else None,
                             v, o, mp)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[k] = r
    return _cache[k]
