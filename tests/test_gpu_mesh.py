"""The grid triangulation on the device (needs an MI355X): sgm_mesh_grid, sgm_mesh_grid_device, Engine.mesh_grid_host / _device,
sgm.triangulate_points.

Yardstick: tests/mesh_ref.py -- the definition of include/sgm_hip_mesh.h in vectorised numpy -- bit for bit: vertices, colours,
faces and both counts.  Every output is pre-filled with a marker, so rows past the counts are seen untouched, and every input is
checked unmodified."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import parity_util as U
import mesh_ref as MR
import voxel_ref as VR
import stereo_reconstruction_cv_amd as sgm
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = dict(numDisparities=16)
NCASE = len(MR.SHAPE_CASES)
MARK_F, MARK_B, MARK_I = np.float32(-77.25), 177, -123456789
STAGES = {"mesh_quads": 1, "mesh_used": 1, "mesh_scan": 2, "mesh_vertices": 1, "mesh_faces": 1, "_wall": 0}


@pytest.fixture(scope="module")
def eng():
    return Engine(P16)


@functools.lru_cache(maxsize=None)
def layered():
    """the 48 x 320 layered cloud, shared and read-only"""
    out = MR.layered_cloud(48, 320, 704)
    for a in out:
        a.setflags(write=False)
    return out


def rows(H, W):
    return max(H * W, 1), max(2 * (H - 1) * (W - 1), 1)


def host(e, xyz, disp, col, md):
    """the host entry called on marked outputs of the worst-case size: (vertices, colors, faces, n_vertices, n_faces), whole arrays"""
    xyz, disp = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(disp, np.float32)
    col = None if col is None else np.ascontiguousarray(col, np.uint8)
    H, W = disp.shape
    keep = [xyz.copy(), disp.copy(), None if col is None else col.copy()]
    nr, fr = rows(H, W)
    vert = np.full((nr, 3), MARK_F, np.float32)
    rgb = None if col is None else np.full((nr, 3), MARK_B, np.uint8)
    faces = np.full((fr, 3), MARK_I, np.int32)
    nv, nf = C.c_int64(-5), C.c_int64(-6)
    at = lambda a: None if a is None else a.ctypes.data
    rc = _lib.load().sgm_mesh_grid(e._h, xyz.ctypes.data, disp.ctypes.data, at(col), H, W, float(md), vert.ctypes.data, at(rgb),
                                   faces.ctypes.data, C.byref(nv), C.byref(nf))
    assert rc == 0, _lib.last_error()
    assert np.array_equal(xyz, keep[0], equal_nan=True) and np.array_equal(disp, keep[1], equal_nan=True)
    assert col is None or np.array_equal(col, keep[2])
    return vert, rgb, faces, nv.value, nf.value


def device(e, xyz, disp, col, md):
    """the same through the device entry, every array a tensor of its own"""
    import torch
    dev = torch.device("cuda", e.device)
    H, W = disp.shape
    up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    dx, dd, dc = up(xyz), up(disp), up(col)
    nr, fr = rows(H, W)
    vert = torch.full((nr, 3), float(MARK_F), dtype=torch.float32, device=dev)
    rgb = None if col is None else torch.full((nr, 3), MARK_B, dtype=torch.uint8, device=dev)
    faces = torch.full((fr, 3), MARK_I, dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    torch.cuda.synchronize()
    nv, nf = e.mesh_grid_device(p(dx), p(dd), p(dc), H, W, md, p(vert), p(rgb), p(faces))
    e.synchronize()
    assert np.array_equal(dx.cpu().numpy(), xyz, equal_nan=True) and np.array_equal(dd.cpu().numpy(), disp, equal_nan=True)
    assert col is None or np.array_equal(dc.cpu().numpy(), col)
    back = lambda t: None if t is None else t.cpu().numpy()
    return back(vert), back(rgb), back(faces), nv, nf


def same(got, want, what=""):
    """bit for bit against a reference result, and the rows behind it untouched"""
    vert, rgb, faces, nv, nf = got
    V, F = want["n_vertices"], want["n_faces"]
    assert (nv, nf) == (V, F), (what, nv, nf, V, F)
    assert vert.dtype == np.float32 and np.array_equal(vert[:V].view(np.uint32), want["vertices"].view(np.uint32)), \
        (what, int((vert[:V].view(np.uint32) != want["vertices"].view(np.uint32)).sum()))
    assert (vert[V:] == MARK_F).all(), what
    if rgb is not None:
        assert rgb.dtype == np.uint8 and np.array_equal(rgb[:V], want["colors"]) and (rgb[V:] == MARK_B).all(), what
    assert faces.dtype == np.int32 and np.array_equal(faces[:F], want["faces"]), (what, int((faces[:F] != want["faces"]).any(axis=1).sum()))
    assert (faces[F:] == MARK_I).all(), what


def both(e, xyz, disp, col, md, want=None, what=""):
    if want is None:
        want = MR.mesh_grid(xyz, disp, col, md)
    same(host(e, xyz, disp, col, md), want, (what, "host"))
    same(device(e, xyz, disp, col, md), want, (what, "device"))
    return want


# ---- 1. shapes, through both entries, with and without colours ------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NCASE))
def test_shapes_through_both_entries(eng, i):
    H, W, md = MR.SHAPE_CASES[i]
    xyz, disp, col = MR.case_input(i)
    for with_col in (True, False):
        want = MR.case_want(i, with_col)
        for fn in (host, device):
            same(fn(eng, xyz, disp, col if with_col else None, md), want, (H, W, fn.__name__, with_col))
    assert (MR.case_want(i)["n_faces"] > 0) == (H >= 2 and W >= 2)


def test_colours_given_but_not_asked_for_are_ignored(eng):
    import torch
    xyz, disp, col = layered()
    H, W = disp.shape
    dx, dd, dc = (torch.from_numpy(np.array(a)).cuda() for a in (xyz, disp, col))
    vert = torch.full((H * W, 3), float(MARK_F), dtype=torch.float32, device="cuda")
    faces = torch.full((2 * (H - 1) * (W - 1), 3), MARK_I, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nv, nf = eng.mesh_grid_device(dx.data_ptr(), dd.data_ptr(), dc.data_ptr(), H, W, 0.25, vert.data_ptr(), None, faces.data_ptr())
    same((vert.cpu().numpy(), None, faces.cpu().numpy(), nv, nf), MR.mesh_grid(xyz, disp, None, 0.25))


def test_images_off_a_16_byte_boundary_give_the_same_bits(eng):
    """48 x 320 has W % 4 == 0, so k_mesh_quads reads 16-byte words -- unless an image starts off a 16-byte boundary: then the
    float-by-float form runs.  Either image 4 bytes off, and both"""
    import torch
    xyz, disp, col = layered()
    H, W = disp.shape
    n = H * W
    want = MR.mesh_grid(xyz, disp, col, 0.25)
    bx = torch.zeros(n * 3 + 4, dtype=torch.float32, device="cuda")
    bd = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    dc = torch.from_numpy(np.array(col)).cuda()
    assert bx.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0
    for ox, od in ((1, 0), (0, 1), (1, 1), (0, 0)):
        bx[ox:ox + n * 3] = torch.from_numpy(np.array(xyz)).cuda().flatten()
        bd[od:od + n] = torch.from_numpy(np.array(disp)).cuda().flatten()
        vert = torch.full((n, 3), float(MARK_F), dtype=torch.float32, device="cuda")
        rgb = torch.full((n, 3), MARK_B, dtype=torch.uint8, device="cuda")
        faces = torch.full((2 * (H - 1) * (W - 1), 3), MARK_I, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        nv, nf = eng.mesh_grid_device(bx.data_ptr() + 4 * ox, bd.data_ptr() + 4 * od, dc.data_ptr(), H, W, 0.25, vert.data_ptr(),
                                      rgb.data_ptr(), faces.data_ptr())
        same((vert.cpu().numpy(), rgb.cpu().numpy(), faces.cpu().numpy(), nv, nf), want, (ox, od))


# ---- 2. extremes at 48 x 320 -----------------------------------------------------------------------------------------------------------
def test_every_pixel_invalid(eng):
    xyz, disp, col = layered()
    assert both(eng, xyz, np.zeros_like(disp), col, 1.0, what="disp 0")["n_faces"] == 0
    bad = np.array(xyz)
    y, x = np.mgrid[0:48, 0:320]
    bad[y, x, (y + x) % 3] = np.nan
    want = both(eng, bad, np.abs(disp) + 1, col, 100.0, what="nan")
    assert (want["n_vertices"], want["n_faces"]) == (0, 0)


def test_a_checkerboard_of_validity_gives_no_triangle_and_no_vertex(eng):
    """every quad has exactly two valid corners, on one diagonal: the diagonal connects and no triangle has a third corner"""
    xyz, disp, col = MR.ramp_cloud(48, 320)
    y, x = np.mgrid[0:48, 0:320]
    disp[(y + x) % 2 == 1] = 0
    want = both(eng, xyz, disp, col, 100.0, what="checkerboard")
    assert (want["n_vertices"], want["n_faces"]) == (0, 0) and want["valid"].sum() == 48 * 320 // 2


def test_the_ramp_in_closed_form(eng):
    H, W = 48, 320
    xyz, disp, col = MR.ramp_cloud(H, W)
    want = dict(vertices=xyz.reshape(-1, 3), colors=col.reshape(-1, 3), faces=MR.ramp_faces(H, W), n_vertices=H * W,
                n_faces=2 * (H - 1) * (W - 1))
    both(eng, xyz, disp, col, 0.0, want=want, what="ramp")


@pytest.mark.parametrize("md", [0.0, 0.125, 0.25, 1.0, 100.0])
def test_max_diff(eng, md):
    xyz, disp, col = layered()
    want = both(eng, xyz, disp, col, md, what=("max_diff", md))
    assert (want["n_faces"] == 0) == (md == 0.0)          # (the noise leaves no two equal neighbours)
    if md == 100.0:
        assert int((want["valid"] & ~want["used"]).sum()) == 8


def test_a_step_edge_below_at_and_above_the_step(eng):
    """left half at 10 pixels, right half at 12.5: the column of quads across the step connects iff max_diff >= 2.5"""
    H, W = 48, 320
    xyz, disp, col = MR.ramp_cloud(H, W, 10.0)
    disp[:, W // 2:] = 12.5
    full = 2 * (H - 1) * (W - 1)
    for md, F in ((2.25, full - 2 * (H - 1)), (2.5, full), (2.75, full)):
        want = both(eng, xyz, disp, col, md, what=("step", md))
        assert (want["n_faces"], want["n_vertices"]) == (F, H * W)


def test_the_tie_frame_tiled_across_a_whole_block(eng):
    """the hand-made quads of test_mesh_reference.py side by side: rows 0 and 1 repeat [160, 168 | 164, 164] (a tie: a-d) with
    every fourth quad turned into the strict b-c case, over 48 x 320 so that ties sit in every lane of many blocks"""
    H, W = 48, 320
    xyz, _, col = MR.ramp_cloud(H, W)
    y, x = np.mgrid[0:H, 0:W]
    six = np.where(y % 2 == 0, np.where(x % 2 == 0, 160, 168), 164).astype(np.float32)
    six[(y % 2 == 1) & (x % 8 == 0)] = 165
    disp = six / np.float32(16)
    want = both(eng, xyz, disp, col, 1.0, what="ties")
    quads_ad, quads_bc = int((~want["bc"]).sum()), int(want["bc"].sum())
    assert quads_ad > 5000 and quads_bc > 1000 and want["n_faces"] == 2 * (H - 1) * (W - 1)
    even = want["bc"][0::2, 0::2]                          # quads with a = 160, b = 168 on top: a-d unless c was raised to 165
    assert not even[:, 1::4].any() and even[:, 0::4].all()


# ---- 3. determinism, history, poison, the stage record ---------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bits(eng):
    xyz, disp, col = layered()
    a, b = device(eng, xyz, disp, col, 0.25), device(eng, xyz, disp, col, 0.25)
    assert a[3:] == b[3:] and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[:3], b[:3]))
    same(a, MR.mesh_grid(xyz, disp, col, 0.25))


def test_results_do_not_depend_on_what_the_engine_did_before():
    e = Engine(P16)
    def run(i, fn):
        xyz, disp, col = MR.case_input(i)
        same(fn(e, xyz, disp, col, MR.SHAPE_CASES[i][2]), MR.case_want(i), (i, fn.__name__))
    big, small = 7, 5                       # 97 x 331, then 3 x 257
    run(small, host)
    run(big, device)
    run(small, device)                      # a smaller frame in the larger maps
    run(big, host)
    e.trim()                                # gives the maps back; they return on the next call
    run(small, device)
    try:
        for byte in (0xA5, 0x7F, 0x00, 0xFF):
            e.set_option(_lib.SGM_OPT_POISON, byte)      # fills every buffer the engine owns and arms the same for new ones
            run(small, host)
            e.set_option(_lib.SGM_OPT_POISON, byte)
            run(big, device)
            run(small, device)
    finally:
        e.set_option(_lib.SGM_OPT_POISON, -1)


def test_the_profile_record_names_the_stages():
    e = Engine(P16)
    xyz, disp, col = layered()
    try:
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        same(device(e, xyz, disp, col, 0.25), MR.mesh_grid(xyz, disp, col, 0.25))
        st = {n: launches for n, ms, launches in e.stage_times()}
        assert st == STAGES, st
    finally:
        e.set_option(_lib.SGM_OPT_PROFILE, 0)


# ---- 4. frames of the size users run ------------------------------------------------------------------------------------------------------
def test_one_1080p_frame_from_the_pipeline():
    """1080 x 1920 through sgm_pipeline_device, then the device entry on the resident XYZ image and float disparity at two
    max_diff"""
    import torch
    H, W, D = 1080, 1920, 128
    a, b = synth.make_pair(H, W, D, seed=5)[:2]
    e = Engine(U.params(D, 5, 0, 1))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dd = torch.empty((H, W), dtype=torch.int16, device="cuda")
    df = torch.empty((H, W), dtype=torch.float32, device="cuda")
    dx = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    rgb = torch.from_numpy(np.repeat(a[:, :, None], 3, axis=2) ^ np.array([0, 85, 170], np.uint8)).cuda()
    torch.cuda.synchronize()
    e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, synth.default_Q(W), dd.data_ptr(), df.data_ptr(), dx.data_ptr())
    e.synchronize()
    xyz, disp, col = dx.cpu().numpy(), df.cpu().numpy(), rgb.cpu().numpy()
    assert MR.valid_mask(xyz, disp).mean() > 0.3
    n, fmax = H * W, 2 * (H - 1) * (W - 1)
    vert = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    oc = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    faces = torch.empty((fmax, 3), dtype=torch.int32, device="cuda")
    seen = []
    for md in (0.5, 2.0):
        want = MR.mesh_grid(xyz, disp, col, md)
        vert.fill_(float(MARK_F)), oc.fill_(MARK_B), faces.fill_(MARK_I)
        torch.cuda.synchronize()
        nv, nf = e.mesh_grid_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), H, W, md, vert.data_ptr(), oc.data_ptr(), faces.data_ptr())
        assert (nv, nf) == (want["n_vertices"], want["n_faces"]) and nf > 100000 and nv < n
        assert np.array_equal(vert[:nv].cpu().numpy().view(np.uint32), want["vertices"].view(np.uint32))
        assert np.array_equal(oc[:nv].cpu().numpy(), want["colors"]) and np.array_equal(faces[:nf].cpu().numpy(), want["faces"])
        assert bool((vert[nv:] == float(MARK_F)).all()) and bool((oc[nv:] == MARK_B).all()) and bool((faces[nf:] == MARK_I).all())
        seen.append(nf)
    assert seen[0] < seen[1]
    assert np.array_equal(dx.cpu().numpy(), xyz, equal_nan=True) and np.array_equal(df.cpu().numpy(), disp, equal_nan=True)


def test_a_4k_class_frame_all_valid_against_the_closed_form():
    """2160 x 4096, every pixel valid and connected: V = 8 847 360 and F = 17 682 210, the largest a frame of this class can have
    (34 560 blocks through the one-workgroup scan, face offsets past 2^24).  The ramp is built on the device; the faces are held
    against the formula there too."""
    import torch
    H, W = 2160, 4096
    n, F = H * W, 2 * (H - 1) * (W - 1)
    assert F == 17682210
    dev = torch.device("cuda")
    yy = torch.arange(H, device=dev, dtype=torch.float32).view(H, 1).expand(H, W)
    xx = torch.arange(W, device=dev, dtype=torch.float32).view(1, W).expand(H, W)
    dx = torch.stack([xx * 0.01, yy * 0.01, torch.full((H, W), 2.0, device=dev)], dim=2).contiguous()
    dd = torch.full((H, W), 8.0, dtype=torch.float32, device=dev)
    dc = (torch.arange(n * 3, device=dev, dtype=torch.int32) % 251).to(torch.uint8).view(H, W, 3)
    vert = torch.full((n, 3), float(MARK_F), dtype=torch.float32, device=dev)
    oc = torch.full((n, 3), MARK_B, dtype=torch.uint8, device=dev)
    faces = torch.full((F + 8, 3), MARK_I, dtype=torch.int32, device=dev)
    e = Engine(P16)
    torch.cuda.synchronize()
    nv, nf = e.mesh_grid_device(dx.data_ptr(), dd.data_ptr(), dc.data_ptr(), H, W, 0.0, vert.data_ptr(), oc.data_ptr(), faces.data_ptr())
    assert (nv, nf) == (n, F)
    assert torch.equal(vert, dx.view(n, 3)) and torch.equal(oc, dc.view(n, 3))
    q = torch.arange((H - 1) * (W - 1), device=dev, dtype=torch.int64)
    a = (q // (W - 1)) * W + q % (W - 1)
    want = torch.stack([a, a + W, a + W + 1, a, a + W + 1, a + 1], dim=1).to(torch.int32).view(F, 3)
    assert torch.equal(faces[:F], want) and bool((faces[F:] == MARK_I).all())


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched_and_the_engine_usable(eng):
    L = _lib.load()
    xyz, disp, col = (np.array(a[:10, :10]) for a in layered())
    H = W = 10
    vert, rgb, faces = np.full((100, 3), MARK_F, np.float32), np.full((100, 3), MARK_B, np.uint8), np.full((162, 3), MARK_I, np.int32)
    nv, nf = C.c_int64(-5), C.c_int64(-6)
    X, D, Cc, P, R, Fp = xyz.ctypes.data, disp.ctypes.data, col.ctypes.data, vert.ctypes.data, rgb.ctypes.data, faces.ctypes.data
    NV, NF = C.byref(nv), C.byref(nf)
    h = eng._h
    bad = [
        (None, X, D, Cc, H, W, 1.0, P, R, Fp, NV, NF), (h, None, D, Cc, H, W, 1.0, P, R, Fp, NV, NF), (h, X, None, Cc, H, W, 1.0, P, R, Fp, NV, NF),
        (h, X, D, Cc, H, W, 1.0, None, R, Fp, NV, NF), (h, X, D, Cc, H, W, 1.0, P, R, None, NV, NF), (h, X, D, Cc, H, W, 1.0, P, R, Fp, None, NF),
        (h, X, D, Cc, H, W, 1.0, P, R, Fp, NV, None),
        (h, X, D, Cc, 0, W, 1.0, P, R, Fp, NV, NF), (h, X, D, Cc, H, 0, 1.0, P, R, Fp, NV, NF), (h, X, D, Cc, -3, W, 1.0, P, R, Fp, NV, NF),
        (h, X, D, Cc, H, W, -1.0, P, R, Fp, NV, NF), (h, X, D, Cc, H, W, float("nan"), P, R, Fp, NV, NF),
        (h, X, D, Cc, H, W, float("inf"), P, R, Fp, NV, NF), (h, X, D, Cc, H, W, -1e-30, P, R, Fp, NV, NF),
        (h, X, D, None, H, W, 1.0, P, R, Fp, NV, NF),
    ]
    for fn in (L.sgm_mesh_grid, L.sgm_mesh_grid_device):
        for args in bad:
            assert fn(*args) == -1, args                                   # SGM_ERR_INVALID_ARG
            assert b"sgm_mesh_grid" in L.sgm_last_error()
        assert fn(h, X, D, Cc, 8193, 8192, 1.0, P, R, Fp, NV, NF) == -4     # SGM_ERR_UNSUPPORTED: before anything is read
        assert b"2^26" in L.sgm_last_error()
    assert (vert == MARK_F).all() and (rgb == MARK_B).all() and (faces == MARK_I).all() and (nv.value, nf.value) == (-5, -6)
    # no quad: success with 0 and 0, nothing read or written
    for fn in (L.sgm_mesh_grid, L.sgm_mesh_grid_device):
        for hh, ww in ((1, 100), (100, 1), (1, 1)):
            nv.value, nf.value = -5, -6
            assert fn(h, X, D, None, hh, ww, 1.0, P, None, Fp, NV, NF) == 0 and (nv.value, nf.value) == (0, 0)
    assert (vert == MARK_F).all() and (faces == MARK_I).all()
    both(eng, *layered(), 0.25, what="after the refusals")


# ---- 6. the existing paths ---------------------------------------------------------------------------------------------------------------
def test_the_compaction_and_the_voxel_grid_are_unchanged_after_a_mesh_call():
    import torch
    e = Engine(P16)
    xyz, disp, col = MR.layered_cloud(97, 331, 9)
    mask = ~np.isnan(xyz[:, :, 0]) & ~np.isinf(xyz[:, :, 0]) & (disp > 0)
    lst = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)
    vox = VR.voxel_downsample(*lst, 0.05)
    both(e, xyz, disp, col, 0.25)
    p, c = e.compact_points_host(xyz, disp, col)
    assert np.array_equal(p.view(np.uint32), xyz[mask].view(np.uint32)) and np.array_equal(c, col[mask])
    n = disp.size
    dx, dd, dc = (torch.from_numpy(a).cuda() for a in (xyz, disp, col))
    op, oc = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    ok = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m = e.compact_points_device(dx.data_ptr(), dd.data_ptr(), dc.data_ptr(), n, op.data_ptr(), oc.data_ptr())
    assert m == int(mask.sum())
    assert np.array_equal(op[:m].cpu().numpy().view(np.uint32), xyz[mask].view(np.uint32)) and np.array_equal(oc[:m].cpu().numpy(), col[mask])
    both(e, xyz, disp, col, 1.0)
    p, c, k, noor = e.voxel_downsample_host(*lst, 0.05, return_counts=True)
    assert noor == vox["n_out_of_range"] and np.array_equal(p.view(np.uint32), vox["points"].view(np.uint32))
    assert np.array_equal(c, vox["colors"]) and np.array_equal(k, vox["counts"])
    nvx, noor = e.voxel_downsample_device(dx.data_ptr(), dd.data_ptr(), dc.data_ptr(), n, 0.05, (0, 0, 0), 1, op.data_ptr(), oc.data_ptr(),
                                          ok.data_ptr())
    assert (nvx, noor) == (vox["n_voxels"], vox["n_out_of_range"])
    assert np.array_equal(op[:nvx].cpu().numpy().view(np.uint32), vox["points"].view(np.uint32))
    assert np.array_equal(oc[:nvx].cpu().numpy(), vox["colors"]) and np.array_equal(ok[:nvx].cpu().numpy().view(np.uint32), vox["counts"])
    sgm.triangulate_points(xyz, col, disp, 0.25)                   # ... and on the default engine, which valid_points uses
    p, c = sgm.valid_points(xyz, col, disp)
    assert np.array_equal(p.view(np.uint32), xyz[mask].view(np.uint32)) and np.array_equal(c, col[mask])
    p, c = sgm.voxel_down_sample(xyz, col, disp, 0.05)
    assert np.array_equal(p.view(np.uint32), vox["points"].view(np.uint32)) and np.array_equal(c, vox["colors"])


# ---- 7. the Python surface -----------------------------------------------------------------------------------------------------------------
def test_triangulate_points_on_numpy_input(tmp_path):
    xyz, disp, col = MR.layered_cloud(48, 320, 31)
    want = MR.mesh_grid(xyz, disp, col, 1.0)
    v, c, t = sgm.triangulate_points(xyz, col, disp)                       # max_diff = 1.0 is the default
    assert v.dtype == np.float32 and c.dtype == np.uint8 and t.dtype == np.int32
    assert np.array_equal(v.view(np.uint32), want["vertices"].view(np.uint32)) and np.array_equal(c, want["colors"])
    assert np.array_equal(t, want["faces"]) and t.shape[0] > 5000
    v, c, t = sgm.triangulate_points(xyz, None, disp, 0.25)
    w2 = MR.mesh_grid(xyz, disp, None, 0.25)
    assert c is None and np.array_equal(v.view(np.uint32), w2["vertices"].view(np.uint32)) and np.array_equal(t, w2["faces"])
    # with a confidence map: the mask of valid_points
    conf = np.random.default_rng(3).integers(0, 101, size=disp.shape).astype(np.uint8)
    w3 = MR.mesh_grid(xyz, np.where(conf >= 40, disp, np.float32(0)), col, 1.0)
    v, c, t = sgm.triangulate_points(xyz, col, disp, 1.0, confidence=conf, min_confidence=40)
    assert 0 < w3["n_faces"] < want["n_faces"]
    assert np.array_equal(v.view(np.uint32), w3["vertices"].view(np.uint32)) and np.array_equal(c, w3["colors"]) and np.array_equal(t, w3["faces"])
    # ... and out to a file and back
    path = str(tmp_path / "m.ply")
    sgm.write_triangle_mesh(path, v, t, c)
    rv, rc, rt = sgm.read_triangle_mesh(path)
    assert np.array_equal(rv, v.astype(np.float64)) and np.array_equal(rc, c) and np.array_equal(rt, t)


# ---- 8. guarded buffers -------------------------------------------------------------------------------------------------------------------
def test_the_cases_with_every_buffer_guarded():
    """(the same cases ran in the plain mode above)"""
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mesh_guard_child.py")], capture_output=True, text=True, env=env,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"MESH_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) >= 12, tail
