"""The grid triangulation of include/sgm_hip_mesh.h, restated in vectorised numpy: the reference the device results are held against
bit for bit (tests/test_gpu_mesh.py), the hand-worked answers of tests/test_mesh_reference.py, the closed form of the ramp frame and
the shape list.  Nothing here knows about blocks, ballots or scans: the quads are whole-array expressions, the vertex numbers a
cumulative sum over the used pixels, and every disparity difference is one numpy float32 subtraction, rounded to binary32."""
import numpy as np

from voxel_ref import layered_cloud  # noqa: F401  (the cloud generator is shared with the voxel tests)

MAX_PIXELS = 1 << 26                 # the header's limit on H * W
F32 = np.float32


def valid_mask(xyz, disp):
    """step 1: X, Y, Z all finite and disp > 0"""
    return np.isfinite(xyz).all(axis=2) & (disp > 0)


def quad_codes(xyz, disp, max_diff):
    """steps 1 .. 3 for every quad: (valid (H, W), bc, first, second (H-1, W-1) bool): the quad takes diagonal b-c (else a-d), it
    emits its first triangle (T0 or T2), its second (T1 or T3).  H, W >= 2."""
    md = F32(max_diff)
    assert np.isfinite(md) and md >= 0
    v = valid_mask(xyz, disp)
    va, vb, vc, vd = v[:-1, :-1], v[:-1, 1:], v[1:, :-1], v[1:, 1:]
    da, db, dc, dd = disp[:-1, :-1], disp[:-1, 1:], disp[1:, :-1], disp[1:, 1:]

    def diff(p, q):
        r = np.abs(p - q)                       # one binary32 subtraction, one absolute value
        assert r.dtype == np.float32
        return r

    with np.errstate(all="ignore"):
        ab, ac, ad, bc, bd, cd = diff(da, db), diff(da, dc), diff(da, dd), diff(db, dc), diff(db, dd), diff(dc, dd)
        cab, cac, cad = va & vb & (ab <= md), va & vc & (ac <= md), va & vd & (ad <= md)     # (a NaN difference compares false)
        cbc, cbd, ccd = vb & vc & (bc <= md), vb & vd & (bd <= md), vc & vd & (cd <= md)
        take_ad = va & vd & (~(vb & vc) | (ad <= bc))
    first = np.where(take_ad, cac & ccd & cad, cac & cbc & cab)      # T0 = (a, c, d)   T2 = (a, c, b)
    second = np.where(take_ad, cad & cbd & cab, cbc & ccd & cbd)     # T1 = (a, d, b)   T3 = (b, c, d)
    return v, ~take_ad, first, second


def mesh_grid(xyz, disp, colors=None, max_diff=1.0):
    """The whole definition.  Returns a dict: vertices float32 (V, 3), colors uint8 (V, 3) or None, faces int32 (F, 3), n_vertices,
    n_faces, and for the tests valid, used (H, W) bool, bc, first, second (H-1, W-1) bool, pixels int64 (V) (each vertex's pixel)."""
    xyz, disp = np.asarray(xyz), np.asarray(disp)
    assert xyz.dtype == np.float32 and xyz.ndim == 3 and xyz.shape[2] == 3
    H, W = xyz.shape[:2]
    assert disp.dtype == np.float32 and disp.shape == (H, W) and 1 <= H * W <= MAX_PIXELS
    if colors is not None:
        colors = np.asarray(colors)
        assert colors.dtype == np.uint8 and colors.shape == (H, W, 3)
    if H < 2 or W < 2:
        e = np.zeros((max(H - 1, 0), max(W - 1, 0)), bool)
        return dict(vertices=np.zeros((0, 3), np.float32), colors=None if colors is None else np.zeros((0, 3), np.uint8),
                    faces=np.zeros((0, 3), np.int32), n_vertices=0, n_faces=0, valid=valid_mask(xyz, disp),
                    used=np.zeros((H, W), bool), bc=e, first=e, second=e, pixels=np.zeros(0, np.int64))
    v, bc, first, second = quad_codes(xyz, disp, max_diff)
    y, x = np.mgrid[0:H - 1, 0:W - 1]
    a = (y * W + x).astype(np.int64)
    b, c, d = a + 1, a + W, a + W + 1
    # the two candidate triangles of every quad in pixel numbers, (H-1, W-1, 2, 3): [.., 0, :] the first, [.., 1, :] the second
    tri = np.stack([np.stack([a, c, np.where(bc, b, d)], axis=2),
                    np.stack([np.where(bc, b, a), np.where(bc, c, d), np.where(bc, d, b)], axis=2)], axis=2)
    emit = np.stack([first, second], axis=2)
    faces_px = tri[emit]                                   # boolean indexing keeps the order: quad row-major, first before second
    used = np.zeros(H * W, bool)
    used[faces_px.reshape(-1)] = True
    number = np.cumsum(used) - 1                           # pixel -> vertex number, on used pixels
    pixels = np.nonzero(used)[0]
    faces = number[faces_px].astype(np.int32).reshape(-1, 3)
    return dict(vertices=xyz.reshape(-1, 3)[pixels], colors=None if colors is None else colors.reshape(-1, 3)[pixels],
                faces=faces, n_vertices=int(pixels.size), n_faces=int(faces.shape[0]), valid=v, used=used.reshape(H, W),
                bc=bc, first=first, second=second, pixels=pixels)


def ramp_cloud(H, W, disparity=8.0):
    """every pixel valid, one disparity: X grows with x, Y with y, Z constant.  (xyz, disp, colors)"""
    y, x = np.mgrid[0:H, 0:W]
    xyz = np.stack([x * 0.01, y * 0.01, np.full((H, W), 2.0)], axis=2).astype(np.float32)
    colors = np.stack([x & 255, y & 255, (x + y) & 255], axis=2).astype(np.uint8)
    return xyz, np.full((H, W), disparity, np.float32), colors


def ramp_faces(H, W):
    """the ramp in closed form: V = H W, every quad takes a-d (a tie), F = 2 (H-1)(W-1); face 2q is T0 = (a, c, d) and face 2q + 1 is
    T1 = (a, d, b) of quad q = y (W-1) + x, a = y W + x"""
    q = np.arange((H - 1) * (W - 1), dtype=np.int64)
    a = (q // (W - 1)) * W + q % (W - 1)
    f = np.empty((q.size, 2, 3), np.int32)
    f[:, 0, 0], f[:, 0, 1], f[:, 0, 2] = a, a + W, a + W + 1
    f[:, 1, 0], f[:, 1, 1], f[:, 1, 2] = a, a + W + 1, a + 1
    return f.reshape(-1, 3)


# (H, W, max_diff): the eight shapes of the issue, then two of our own.  The kernels walk the pixels in row-major order in blocks of
# 1024 and waves of 64 and do not tile; k_mesh_quads gives a lane four pixels and reads them as 16-byte words where W % 4 == 0.
#   1 x 1 and 1 x 64 have no quad, 2 x 2 one; 2 x 63 / 2 x 65 put the row below under / past 64 pixels; 3 x 257 is ragged in every
#   group of four; 48 x 320 (wide loads) and 97 x 331 (not) have many blocks and a ragged last one; 3 x 1028 (wide) and 2 x 1025
#   (not) put the row below past a block.  Case i is layered_cloud(H, W, 700 + i).
SHAPE_CASES = [
    (1, 1, 0.25),
    (1, 64, 0.25),
    (2, 2, 100.0),
    (2, 63, 1.0),
    (2, 65, 0.25),
    (3, 257, 1.0),
    (48, 320, 0.25),
    (97, 331, 0.25),
    (3, 1028, 2.0),
    (2, 1025, 1.0),
]


def case_input(i):
    H, W = SHAPE_CASES[i][:2]
    return layered_cloud(H, W, 700 + i)


_cache = {}


def want(xyz, disp, colors, max_diff):
    """mesh_grid with its arrays made read-only"""
    r = mesh_grid(xyz, disp, colors, max_diff)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def case_want(i, with_colors=True):
    """the reference of shape case i, computed once and shared (read-only)"""
    k = (i, with_colors)
    if k not in _cache:
        xyz, disp, col = case_input(i)
        _cache[k] = want(xyz, disp, col if with_colors else None, SHAPE_CASES[i][2])
    return _cache[k]
