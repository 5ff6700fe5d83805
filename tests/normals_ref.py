"""The vertex normals of include/sgm_hip_normals.h, restated in numpy on top of mesh_ref.quad_codes -- twice, so that the order of
the additions is pinned twice: normal_image is whole-array expressions, eight masked additions in face order; normal_image_loop is
a plain Python loop over the pixels that follows steps 6 - 9 of the header literally, for small frames.  Every step is one numpy
float32 operation, rounded to binary32 on its own; numpy's float32 division and square root are the correctly rounded ones.  The
device results are held against normal_image bit for bit (tests/test_gpu_normals.py); the two forms against each other and against
answers worked by hand in tests/test_normals_reference.py."""
import numpy as np

import mesh_ref as MR

F32 = np.float32
ZERO = F32(0)


def _face(p, q, r):
    """step 6 on arrays (..., 3): e1 = q - p, e2 = r - p, their cross product with every product and difference rounded"""
    e1, e2 = q - p, r - p
    n = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1],
                  e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                  e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], axis=-1)
    assert n.dtype == np.float32
    return n


def incident(xyz, disp, max_diff):
    """(valid, bc, first, second, steps): steps is the list of step 7's eight additions in their order, each (rows, columns,
    mask (H-1, W-1)): the pixels [rows, columns] take the triangle (first: k % 2 == 0, second: k % 2 == 1) of the quads where mask"""
    v, bc, first, second = MR.quad_codes(xyz, disp, max_diff)
    lo, hi = slice(None, -1), slice(1, None)
    # T0 = (a, c, d) names all but b, T1 = (a, d, b) all but c, T2 = (a, c, b) all but d, T3 = (b, c, d) all but a
    steps = [(hi, hi, first & ~bc), (hi, hi, second),          # the quad above left: the pixel is its d
             (hi, lo, first), (hi, lo, second & bc),           # the quad above: c
             (lo, hi, first & bc), (lo, hi, second),           # the quad to the left: b
             (lo, lo, first), (lo, lo, second & ~bc)]          # its own quad: a
    return v, bc, first, second, steps


def incident_counts(xyz, disp, max_diff):
    """per pixel, how many emitted triangles name it (0 .. 8)"""
    H, W = disp.shape
    k = np.zeros((H, W), np.int64)
    if H >= 2 and W >= 2:
        for ys, xs, on in incident(xyz, disp, max_diff)[4]:
            k[ys, xs] += on
    return k


def _finish(s, used, xyz, orient):
    """steps 8 and 9 on the sums s (H, W, 3)"""
    with np.errstate(all="ignore"):
        m = np.maximum(np.maximum(np.abs(s[..., 0]), np.abs(s[..., 1])), np.abs(s[..., 2]))      # (np.maximum hands a NaN on)
        ok = used & np.isfinite(m) & (m > 0)
        u = s / m[..., None]
        l = np.sqrt((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])
        n = u / l[..., None]
        assert u.dtype == l.dtype == n.dtype == np.float32
        n = np.where(ok[..., None], n, ZERO)
        if orient:
            t = (n[..., 0] * xyz[..., 0] + n[..., 1] * xyz[..., 1]) + n[..., 2] * xyz[..., 2]
            n = np.where((ok & (t > 0))[..., None], np.negative(n), n)
    return n


def normal_image(xyz, disp, max_diff=1.0, orient=1):
    """The whole definition, vectorised: float32 (H, W, 3), +0 on the pixels that are no vertex"""
    xyz, disp = np.asarray(xyz), np.asarray(disp)
    assert xyz.dtype == np.float32 and disp.dtype == np.float32 and xyz.shape == disp.shape + (3,) and orient in (0, 1)
    H, W = disp.shape
    s = np.zeros((H, W, 3), np.float32)
    used = np.zeros((H, W), bool)
    if H < 2 or W < 2:
        return s
    _, bc, first, second, steps = incident(xyz, disp, max_diff)
    a, b, c, d = xyz[:-1, :-1], xyz[:-1, 1:], xyz[1:, :-1], xyz[1:, 1:]
    k = bc[..., None]
    with np.errstate(all="ignore"):
        n1 = _face(a, c, np.where(k, b, d))                                    # T0 = (a, c, d)   T2 = (a, c, b)
        n2 = _face(np.where(k, b, a), np.where(k, c, d), np.where(k, d, b))    # T1 = (a, d, b)   T3 = (b, c, d)
        for j, (ys, xs, on) in enumerate(steps):
            # (a sum is never -0, so adding +0 where the triangle is not the pixel's leaves it as it is)
            s[ys, xs] = s[ys, xs] + np.where(on[..., None], n2 if j % 2 else n1, ZERO)
            used[ys, xs] |= on
    return _finish(s, used, xyz, orient)


def normal_image_loop(xyz, disp, max_diff=1.0, orient=1):
    """The same, one pixel and one float32 operation at a time, as the header writes it.  For small frames."""
    xyz, disp = np.asarray(xyz), np.asarray(disp)
    H, W = disp.shape
    out = np.zeros((H, W, 3), np.float32)
    if H < 2 or W < 2:
        return out
    _, bc, first, second = MR.quad_codes(xyz, disp, max_diff)

    def triangles(qy, qx, me):
        """the emitted triangles of quad (qy, qx) that name its corner `me`, as pixel triples, first before second"""
        if not (0 <= qy < H - 1 and 0 <= qx < W - 1):
            return
        a, b, c, d = (qy, qx), (qy, qx + 1), (qy + 1, qx), (qy + 1, qx + 1)
        both = ((a, c, b), (b, c, d)) if bc[qy, qx] else ((a, c, d), (a, d, b))
        for t, on in zip(both, (first[qy, qx], second[qy, qx])):
            if on and {"a": a, "b": b, "c": c, "d": d}[me] in t:
                yield t

    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                s = [ZERO, ZERO, ZERO]
                vertex = False
                for qy, qx, me in ((y - 1, x - 1, "d"), (y - 1, x, "c"), (y, x - 1, "b"), (y, x, "a")):
                    for tp, tq, tr in triangles(qy, qx, me):
                        p, q, r = xyz[tp], xyz[tq], xyz[tr]
                        e1 = [q[0] - p[0], q[1] - p[1], q[2] - p[2]]
                        e2 = [r[0] - p[0], r[1] - p[1], r[2] - p[2]]
                        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
                        s = [s[0] + n[0], s[1] + n[1], s[2] + n[2]]
                        vertex = True
                assert all(type(v) is np.float32 for v in s)
                m = max(abs(s[0]), abs(s[1]), abs(s[2])) if not any(np.isnan(v) for v in s) else F32(np.nan)
                if not vertex or m == 0 or np.isinf(m) or np.isnan(m):
                    continue
                u = [s[0] / m, s[1] / m, s[2] / m]
                l = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
                n = [u[0] / l, u[1] / l, u[2] / l]
                assert type(l) is np.float32 and all(type(v) is np.float32 for v in n)
                if orient:
                    P = xyz[y, x]
                    t = (n[0] * P[0] + n[1] * P[1]) + n[2] * P[2]
                    if t > 0:
                        n = [-n[0], -n[1], -n[2]]
                out[y, x] = n
    return out


def mesh_grid_normals(xyz, disp, colors=None, max_diff=1.0, orient=1):
    """mesh_ref.mesh_grid and beside it `image` (H, W, 3) and `normals` (V, 3), the image's rows at the vertices' pixels"""
    r = dict(MR.mesh_grid(xyz, disp, colors, max_diff))
    r["image"] = normal_image(xyz, disp, max_diff, orient)
    r["normals"] = r["image"].reshape(-1, 3)[r["pixels"]]
    return r


def exact_plane(H, W, disparity=8.0):
    """X = x 2^-7, Y = y 2^-7, Z = 2 + x 2^-9 + y 2^-10: every input, edge, product and sum of steps 6 and 7 is exact, every face
    normal is (2^-16, 2^-17, -2^-14), and a sum of k of them divided by its largest component is (1/4, 1/8, -1) for every k.
    (xyz, disp)"""
    y, x = np.mgrid[0:H, 0:W]
    xyz = np.stack([x * 2.0 ** -7, y * 2.0 ** -7, 2 + x * 2.0 ** -9 + y * 2.0 ** -10], axis=2)
    assert np.array_equal(xyz.astype(np.float32).astype(np.float64), xyz)
    return xyz.astype(np.float32), np.full((H, W), disparity, np.float32)


def exact_plane_normal():
    """the one normal of the exact plane, by steps 8 and 9 in float32 (t < 0: Z >= 2 and the normal points at the camera)"""
    u = np.array([0.25, 0.125, -1.0], np.float32)
    l = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    return u / l


def mixed_orientation_cloud(H=48, W=320, seed=706):
    """the layered cloud with 2 subtracted from Z: the layer at 1.2 lies behind the origin, the layer at 3.1 in front of it and the
    layer at 2 across it, so that step 9 turns some normals and leaves others.  (xyz, disp, colors)"""
    xyz, disp, col = MR.layered_cloud(H, W, seed)
    xyz = xyz.copy()
    xyz[..., 2] = xyz[..., 2] - F32(2.0)
    return xyz, disp, col


_cache = {}


def case_want(i, orient):
    """mesh_grid_normals of mesh_ref's shape case i with colours, computed once and shared (read-only)"""
    k = (i, orient)
    if k not in _cache:
        xyz, disp, col = MR.case_input(i)
        r = mesh_grid_normals(xyz, disp, col, MR.SHAPE_CASES[i][2], orient)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[k] = r
    return _cache[k]
