"""The truncated signed distance volume of include/sgm_hip_tsdf.h, restated in numpy -- the reference the device results are held
against bit for bit (tests/test_gpu_tsdf.py), the hand-worked answers of tests/test_tsdf_reference.py, the case table and the scene
generators.  Each part is stated twice: `integrate` over whole arrays (with a z-range, so that slabs of a large volume can be checked)
and `integrate_loop` voxel by voxel; `extract_loop` as a plain walk over voxels and axes and `extract` over arrays.  Nothing here
knows about a wave or a launch shape.  Every binary32 step is one numpy float32 operation; the fused multiply-adds are plane_ref's
exact emulation; the sums are integers."""
import numpy as np

import plane_ref as PR

F32 = np.float32
F64 = np.float64
MAX_WEIGHT = 65535
MAX_DIM = 4096
STATS = ("updated", "unclamped", "no_depth", "occluded", "saturated", "outside", "usable_pixels")
fmaf = PR.fmaf


def kappa_of(tau):
    """step 6: formed once, in binary32"""
    return F32(32767.0) / F32(tau)


def empty(dims, color=True):
    """the empty volume: (sum int32 (V), weight int32 (V), rgb_sum uint32 (3, V) or None)"""
    V = int(dims[0]) * int(dims[1]) * int(dims[2])
    return np.zeros(V, np.int32), np.zeros(V, np.int32), (np.zeros((3, V), np.uint32) if color else None)


def m_of(ext):
    """the first three rows of the extrinsic rounded to binary32, (3, 4)"""
    return np.asarray(ext, F64).reshape(4, 4)[:3].astype(F32)


def centre(idx, vs, o):
    """step 1"""
    return fmaf(np.asarray(idx).astype(F32) + F32(0.5), F32(vs), F32(o))


def camera_point(M, cx, cy, cz):
    """step 2: three fused multiply-adds per coordinate, from the translation"""
    return [fmaf(M[a, 2], cz, fmaf(M[a, 1], cy, fmaf(M[a, 0], cx, M[a, 3]))) for a in range(3)]


def usable_pixels(xyz, disp, front, max_depth):
    """step 5 for every pixel: bool (H * W)"""
    p = np.asarray(xyz, F32).reshape(-1, 3)
    fr = F32(front)
    with np.errstate(all="ignore"):
        ok = np.isfinite(p).all(axis=1)
        if disp is not None:
            ok &= np.asarray(disp, F32).reshape(-1) > 0
        d = fr * p[:, 2]
        return ok & (d > 0) & (d <= F32(max_depth))


def integrate(dims, vs, tau, origin, sum_, weight, rgb, xyz, disp, colors, cam, front, ext, max_depth=np.inf, z0=0, z1=None):
    """steps 1 to 7 over arrays, IN PLACE on planes that hold the slabs z0 .. z1 - 1 only (the whole volume by default: sum, weight
    (nx ny (z1 - z0)), rgb (3, the same) or None).  Returns the eight counts of the header, the first six over those slabs."""
    nx, ny, nz = (int(v) for v in dims)
    z1 = nz if z1 is None else z1
    xyz = np.asarray(xyz, F32)
    H, W = xyz.shape[:2]
    pts = xyz.reshape(-1, 3)
    vs, tau, fr = F32(vs), F32(tau), F32(front)
    kappa = kappa_of(tau)
    fx, fy, cx0, cy0 = (F32(v) for v in cam)
    M = m_of(ext)
    k, j, i = np.meshgrid(np.arange(z0, z1), np.arange(ny), np.arange(nx), indexing="ij")
    i, j, k = i.reshape(-1), j.reshape(-1), k.reshape(-1)
    cx, cy, cz = centre(i, vs, origin[0]), centre(j, vs, origin[1]), centre(k, vs, origin[2])
    px, py, pz = camera_point(M, cx, cy, cz)
    with np.errstate(all="ignore"):
        infront = fr * pz > 0
        iz = F32(1.0) / pz
        u = fmaf(fx, px * iz, cx0) + F32(0.5)
        w = fmaf(fy, py * iz, cy0) + F32(0.5)
        inside = infront & (u >= 0) & (u < F32(W)) & (w >= 0) & (w < F32(H))
        qx = np.floor(np.where(inside, u, F32(0))).astype(np.int64)
        qy = np.floor(np.where(inside, w, F32(0))).astype(np.int64)
        pix = qy * W + qx
        usable = usable_pixels(xyz, disp, front, max_depth)
        Z = pts[pix, 2]
        has = inside & usable[pix]
        s = fr * (Z - pz)
        occluded = has & (s < -tau)
        t = np.fmin(s, tau)
        q = np.rint(np.where(has, t * kappa, F32(0))).astype(np.int32)
    cand = has & ~occluded
    saturated = cand & (weight == MAX_WEIGHT)
    upd = cand & ~saturated
    sum_[upd] += q[upd]
    weight[upd] += 1
    if rgb is not None:
        col = np.asarray(colors, np.uint8).reshape(-1, 3)
        for c in range(3):
            rgb[c][upd] += col[pix[upd], c].astype(np.uint32)
    with np.errstate(all="ignore"):
        unclamped = upd & (s < tau)
    return np.array([upd.sum(), unclamped.sum(), (inside & ~has).sum(), occluded.sum(), saturated.sum(), (~inside).sum(), usable.sum(), 0],
                    np.uint64)


def integrate_loop(dims, vs, tau, origin, sum_, weight, rgb, xyz, disp, colors, cam, front, ext, max_depth=np.inf, z0=0, z1=None):
    """the same voxel by voxel, the header's steps one after the other; with the same z-range (the planes hold slabs z0 .. z1 - 1)"""
    nx, ny, nz = (int(v) for v in dims)
    z1 = nz if z1 is None else z1
    xyz = np.asarray(xyz, F32)
    H, W = xyz.shape[:2]
    vs, tau, fr, md = F32(vs), F32(tau), F32(front), F32(max_depth)
    kappa = kappa_of(tau)
    fx, fy, cx0, cy0 = (F32(v) for v in cam)
    M = m_of(ext)
    st = [0] * 8
    with np.errstate(all="ignore"):
        for pix in range(H * W):
            X, Y, Z = xyz.reshape(-1, 3)[pix]
            if np.isfinite(X) and np.isfinite(Y) and np.isfinite(Z) and (disp is None or np.asarray(disp, F32).reshape(-1)[pix] > 0) \
                    and fr * Z > 0 and fr * Z <= md:
                st[6] += 1
        for k in range(z0, z1):
            for j in range(ny):
                for i in range(nx):
                    v = ((k - z0) * ny + j) * nx + i
                    c = [F32(fmaf(F32(n) + F32(0.5), vs, F32(o))) for n, o in zip((i, j, k), origin)]
                    p = [F32(fmaf(M[a, 2], c[2], fmaf(M[a, 1], c[1], fmaf(M[a, 0], c[0], M[a, 3])))) for a in range(3)]
                    if not fr * p[2] > 0:
                        st[5] += 1
                        continue
                    iz = F32(1.0) / p[2]
                    u = F32(fmaf(fx, p[0] * iz, cx0)) + F32(0.5)
                    w = F32(fmaf(fy, p[1] * iz, cy0)) + F32(0.5)
                    if not (u >= 0 and u < F32(W) and w >= 0 and w < F32(H)):
                        st[5] += 1
                        continue
                    pix = int(np.floor(w)) * W + int(np.floor(u))
                    X, Y, Z = xyz.reshape(-1, 3)[pix]
                    ok = np.isfinite(X) and np.isfinite(Y) and np.isfinite(Z) and (disp is None or np.asarray(disp, F32).reshape(-1)[pix] > 0)
                    if not (ok and fr * Z > 0 and fr * Z <= md):
                        st[2] += 1
                        continue
                    s = fr * (Z - p[2])
                    if s < -tau:
                        st[3] += 1
                        continue
                    q = int(np.rint(np.fmin(s, tau) * kappa))
                    if weight[v] == MAX_WEIGHT:
                        st[4] += 1
                        continue
                    sum_[v] += q
                    weight[v] += 1
                    if rgb is not None:
                        for ch in range(3):
                            rgb[ch][v] += np.uint32(np.asarray(colors, np.uint8).reshape(-1, 3)[pix, ch])
                    st[0] += 1
                    st[1] += int(s < tau)
    return np.array(st, np.uint64)


def _colour(rgb, weight, v):
    """the rounded mean of each channel, in integers: uint8 (n, 3)"""
    w = weight[v].astype(np.int64)
    return np.stack([((2 * rgb[c][v].astype(np.int64) + w) // (2 * w)).astype(np.uint8) for c in range(3)], axis=1)


def extract_loop(dims, vs, origin, sum_, weight, rgb, min_weight=1):
    """the crossings by a plain walk: voxel v ascending, axis x, y, z.  (points float32 (n, 3), colours uint8 (n, 3) or None)"""
    nx, ny, nz = (int(v) for v in dims)
    vs = F32(vs)
    step = (1, nx, nx * ny)
    P, Cc = [], []
    with np.errstate(all="ignore"):
        for v in range(nx * ny * nz):
            if weight[v] < min_weight:
                continue
            idx = (v % nx, (v // nx) % ny, v // (nx * ny))
            c = [F32(fmaf(F32(n) + F32(0.5), vs, F32(o))) for n, o in zip(idx, origin)]
            for a in range(3):
                if idx[a] + 1 >= (nx, ny, nz)[a]:
                    continue
                v1 = v + step[a]
                if weight[v1] < min_weight or (sum_[v] < 0) == (sum_[v1] < 0):
                    continue
                f0 = F32(sum_[v]) / F32(weight[v])
                f1 = F32(sum_[v1]) / F32(weight[v1])
                theta = f0 / (f0 - f1)
                p = list(c)
                p[a] = F32(fmaf(theta, vs, c[a]))
                P.append(p)
                if rgb is not None:
                    vc = v if theta <= F32(0.5) else v1
                    w = int(weight[vc])
                    Cc.append([((2 * int(rgb[ch][vc]) + w) // (2 * w)) & 255 for ch in range(3)])
    pts = np.array(P, F32).reshape(-1, 3)
    return pts, (np.array(Cc, np.uint8).reshape(-1, 3) if rgb is not None else None)


def extract(dims, vs, origin, sum_, weight, rgb, min_weight=1, with_axis=False):
    """the same over arrays: only the voxels with weight >= min_weight are looked at, so a large, mostly empty volume is cheap.
    with_axis: a third result, the axis (0, 1, 2) of every crossing"""
    nx, ny, nz = (int(v) for v in dims)
    vs = F32(vs)
    step = (1, nx, nx * ny)
    cand = np.flatnonzero(weight >= min_weight)
    idx = (cand % nx, (cand // nx) % ny, cand // (nx * ny))
    neg = sum_[cand] < 0
    keys, pts, cols = [], [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            has = idx[a] + 1 < (nx, ny, nz)[a]
            v = cand[has]
            v1 = v + step[a]
            ok = (weight[v1] >= min_weight) & ((sum_[v1] < 0) != neg[has])
            v, v1 = v[ok], v1[ok]
            f0 = sum_[v].astype(F32) / weight[v].astype(F32)
            f1 = sum_[v1].astype(F32) / weight[v1].astype(F32)
            theta = f0 / (f0 - f1)
            c = [centre(idx[b][has][ok], vs, origin[b]) for b in range(3)]
            c[a] = fmaf(theta, vs, c[a])
            pts.append(np.stack(c, axis=1).astype(F32).reshape(-1, 3))
            keys.append(v * 3 + a)
            if rgb is not None:
                cols.append(_colour(rgb, weight, np.where(theta <= F32(0.5), v, v1)))
    order = np.argsort(np.concatenate(keys), kind="stable")
    P = np.concatenate(pts)[order]
    C = np.concatenate(cols)[order] if rgb is not None else None
    return (P, C, (np.concatenate(keys)[order] % 3).astype(np.int32)) if with_axis else (P, C)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def rigid(axis, degrees, t):
    """a rigid transformation in float64: the rotation by `degrees` about `axis`, then the translation t"""
    a = np.asarray(axis, F64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


EXTRINSICS = (np.eye(4), rigid((0.2, 1.0, 0.1), 12.0, (0.4, -0.3, 0.5)), rigid((1.0, -0.3, 0.5), -9.0, (-0.6, 0.2, -0.4)))
DEPTH = 10.0          # |Z| of the scenes' wall on the optical axis


def camera_for(H, W):
    """(fx, fy, cx, cy): the focal length 60 at 64 columns, scaled with the width; the principal point a little off the middle"""
    f = 60.0 * W / 64.0
    return (F32(f), F32(f * 1.03125), F32((W - 1) / 2.0 + 0.25), F32((H - 1) / 2.0 - 0.125))


def make_frame(H, W, front=1, seed=0, slope=(0.15, -0.1), noise=0.0, invalid=True, box=True, depth=DEPTH):
    """(xyz float32 (H, W, 3), disp float32 (H, W), colors uint8 (H, W, 3)): a slanted wall at |Z| = depth on the axis, a nearer box over
    part of it, disparity noise of `noise` (baseline 1), and -- with `invalid` -- a few pixels with NaN, inf and disp <= 0."""
    rng = np.random.default_rng(1000 + seed)
    fx, fy, cx, cy = (float(v) for v in camera_for(H, W))
    y, x = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    rx, ry = (x - cx) / fx, (y - cy) / fy
    za = depth / (1.0 - slope[0] * rx - slope[1] * ry)
    if box and H * W > 1:
        inb = (x >= W * 0.55) & (x < W * 0.85) & (y >= H * 0.2) & (y < H * 0.6)
        za = np.where(inb, depth - 1.75, za)
    d = fx / za
    if noise:
        d = d + rng.normal(0.0, noise, d.shape)
    za = fx / d
    Z = front * za
    xyz = np.stack([rx * Z, ry * Z, Z], axis=2).astype(F32)
    disp = d.astype(F32)
    colors = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if invalid and H * W >= 15:
        n = H * W
        bad = rng.permutation(n)[:max(4, n // 12)]
        flat, dflat = xyz.reshape(-1, 3), disp.reshape(-1)
        for t, p in enumerate(bad):
            if t % 4 == 0:
                flat[p, t % 3] = np.nan
            elif t % 4 == 1:
                flat[p, 2] = np.inf * front
            elif t % 4 == 2:
                dflat[p] = 0.0
            else:
                dflat[p] = -1.0
    return xyz, disp, colors


def volume_for(dims, ext, front=1, extent=(10.0, 8.0, 6.0), depth=DEPTH):
    """(voxel_size, origin float32 (3)) of a volume of `dims` voxels whose middle is the wall's point on the optical axis under the
    extrinsic `ext`, and whose size along its longest axis is about the scene's extent there (wider than the frustum: some voxels
    are outside)"""
    vs = F32(max(e / n for e, n in zip(extent, dims)) if max(dims) > 1 else 0.5)
    if dims[1] * dims[2] <= 6 and max(dims) > 1:          # a thin volume lies inside the frustum: both ends of its rows are updated
        vs = F32(6.0 / max(dims))
    ext = np.asarray(ext, F64)
    mid = np.linalg.inv(ext) @ np.array([0.0, 0.0, front * depth, 1.0])
    origin = (mid[:3] - 0.5 * np.asarray(dims, F64) * float(vs)).astype(F32)
    return vs, origin


VOLUMES = ((1, 1, 1), (63, 3, 2), (64, 1, 1), (65, 3, 2), (40, 32, 24))
FRAMES = ((1, 1), (3, 5), (48, 64))
TAU = F32(1.0)


def cases():
    """the case table: (dims, (H, W), extrinsic number, front, color, with_disp), every volume with every frame, the extrinsics, the
    fronts and the options going round"""
    out = []
    n = 0
    for dims in VOLUMES:
        for hw in FRAMES:
            out.append((dims, hw, n % 3, 1 if n % 2 == 0 else -1, n % 4 < 2, n % 3 != 1))
            n += 1
    out += [((40, 32, 24), (48, 64), 1, -1, True, True), ((40, 32, 24), (48, 64), 2, 1, False, False),
            ((65, 3, 2), (48, 64), 1, 1, True, False), ((63, 3, 2), (48, 64), 2, -1, False, True)]
    return out


def case_input(case, seed=0, noise=0.05):
    """the arguments of one integration of a case: a dict of dims, vs, tau, origin, xyz, disp, colors, cam, front, ext"""
    dims, (H, W), en, front, color, with_disp = case
    ext = EXTRINSICS[en]
    xyz, disp, colors = make_frame(H, W, front, seed=seed, noise=noise)
    vs, origin = volume_for(dims, ext, front)
    return dict(dims=dims, vs=vs, tau=TAU, origin=origin, xyz=xyz, disp=disp if with_disp else None, colors=colors if color else None,
                cam=camera_for(H, W), front=front, ext=ext)


def run_case(a, planes=None, fn=integrate, **kw):
    """one integration of case_input's dict into `planes` (a new empty volume by default): (planes, stats)"""
    if planes is None:
        planes = empty(a["dims"], a["colors"] is not None)
    st = fn(a["dims"], a["vs"], a["tau"], a["origin"], planes[0], planes[1], planes[2], a["xyz"], a["disp"], a["colors"], a["cam"], a["front"],
            a["ext"], **kw)
    return planes, st


# ---- the quality scene of the issue ------------------------------------------------------------------------------------------------
def quality_rms(frames, seed0=0, sigma=0.15):
    """A 48 x 64 frame of a fronto-parallel plane at Z = 10, f = 60, disparity noise sigma, a 40 x 32 x 24 volume of 0.25 voxels,
    trunc 1.0: the rms Z error of the extracted crossings after `frames` noisy frames."""
    dims, vs, tau = (40, 32, 24), F32(0.25), F32(1.0)
    origin = np.array([-5.0, -4.0, 7.0], F32)
    planes = empty(dims, False)
    H, W = 48, 64
    cam = (F32(60), F32(60), F32(31.5), F32(23.5))
    for k in range(frames):
        rng = np.random.default_rng(77 + seed0 + k)
        y, x = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
        d = 60.0 / 10.0 + rng.normal(0.0, sigma, (H, W))
        Z = 60.0 / d
        xyz = np.stack([(x - 31.5) / 60.0 * Z, (y - 23.5) / 60.0 * Z, Z], axis=2).astype(F32)
        integrate(dims, vs, tau, origin, planes[0], planes[1], None, xyz, d.astype(F32), None, cam, 1, np.eye(4))
    pts, _ = extract(dims, vs, origin, planes[0], planes[1], None, 1)
    return float(np.sqrt(np.mean((pts[:, 2].astype(F64) - 10.0) ** 2))), pts.shape[0]
