"""The vertex normals on the device (needs an MI355X): sgm_normals_grid, sgm_normals_grid_device, sgm_mesh_grid_normals,
sgm_mesh_grid_normals_device, the Engine methods, sgm.estimate_normals and sgm.triangulate_points_with_normals.

Yardstick: tests/normals_ref.py -- the definition of include/sgm_hip_normals.h in numpy -- bit for bit (as uint32, so that -0
against +0 counts): the normal image, the normal list, and beside the list the mesh of tests/mesh_ref.py.  Every output is
pre-filled with a marker, so rows past the counts are seen untouched, and every input is checked unmodified."""
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
import normals_ref as NR
import voxel_ref as VR
import stereo_reconstruction_cv_amd as sgm
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd.stereo import Engine
from test_gpu_mesh import MARK_B, MARK_F, MARK_I, STAGES, rows, same as same_mesh
from test_gpu_mesh import device as mesh_device, host as mesh_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = dict(numDisparities=16)
NCASE = len(MR.SHAPE_CASES)
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def eng():
    return Engine(P16)


@functools.lru_cache(maxsize=None)
def layered():
    out = MR.layered_cloud(48, 320, 704)
    for a in out:
        a.setflags(write=False)
    return out


def image_host(e, xyz, disp, md, orient):
    xyz, disp = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(disp, np.float32)
    H, W = disp.shape
    keep = xyz.copy(), disp.copy()
    out = np.full((H, W, 3), MARK_F, np.float32)
    rc = _lib.load().sgm_normals_grid(e._h, xyz.ctypes.data, disp.ctypes.data, H, W, float(md), int(orient), out.ctypes.data)
    assert rc == 0, _lib.last_error()
    assert np.array_equal(xyz, keep[0], equal_nan=True) and np.array_equal(disp, keep[1], equal_nan=True)
    return out


def image_device(e, xyz, disp, md, orient):
    import torch
    dev = torch.device("cuda", e.device)
    H, W = disp.shape
    dx, dd = torch.from_numpy(np.array(xyz)).to(dev), torch.from_numpy(np.array(disp)).to(dev)
    out = torch.full((H * W + 1, 3), float(MARK_F), dtype=torch.float32, device=dev)      # one row more: it stays as it is
    torch.cuda.synchronize()
    e.normals_grid_device(dx.data_ptr(), dd.data_ptr(), H, W, md, orient, out.data_ptr())
    e.synchronize()
    assert np.array_equal(dx.cpu().numpy(), xyz, equal_nan=True) and np.array_equal(dd.cpu().numpy(), disp, equal_nan=True)
    got = out.cpu().numpy()
    assert (got[H * W:] == MARK_F).all()
    return got[:H * W].reshape(H, W, 3)


def list_host(e, xyz, disp, col, md, orient):
    """sgm_mesh_grid_normals on marked outputs of the worst-case size: ((vertices, colors, faces, nv, nf), normals)"""
    xyz, disp = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(disp, np.float32)
    col = None if col is None else np.ascontiguousarray(col, np.uint8)
    H, W = disp.shape
    keep = xyz.copy(), disp.copy()
    nr, fr = rows(H, W)
    vert, nrm = np.full((nr, 3), MARK_F, np.float32), np.full((nr, 3), MARK_F, np.float32)
    rgb = None if col is None else np.full((nr, 3), MARK_B, np.uint8)
    faces = np.full((fr, 3), MARK_I, np.int32)
    nv, nf = C.c_int64(-5), C.c_int64(-6)
    at = lambda a: None if a is None else a.ctypes.data
    rc = _lib.load().sgm_mesh_grid_normals(e._h, xyz.ctypes.data, disp.ctypes.data, at(col), H, W, float(md), int(orient), vert.ctypes.data,
                                           at(rgb), faces.ctypes.data, nrm.ctypes.data, C.byref(nv), C.byref(nf))
    assert rc == 0, _lib.last_error()
    assert np.array_equal(xyz, keep[0], equal_nan=True) and np.array_equal(disp, keep[1], equal_nan=True)
    return (vert, rgb, faces, nv.value, nf.value), nrm


def list_device(e, xyz, disp, col, md, orient):
    import torch
    dev = torch.device("cuda", e.device)
    H, W = disp.shape
    up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    dx, dd, dc = up(xyz), up(disp), up(col)
    nr, fr = rows(H, W)
    vert = torch.full((nr, 3), float(MARK_F), dtype=torch.float32, device=dev)
    nrm = torch.full((nr, 3), float(MARK_F), dtype=torch.float32, device=dev)
    rgb = None if col is None else torch.full((nr, 3), MARK_B, dtype=torch.uint8, device=dev)
    faces = torch.full((fr, 3), MARK_I, dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    torch.cuda.synchronize()
    nv, nf = e.mesh_grid_normals_device(p(dx), p(dd), p(dc), H, W, md, orient, p(vert), p(rgb), p(faces), p(nrm))
    e.synchronize()
    assert np.array_equal(dx.cpu().numpy(), xyz, equal_nan=True) and np.array_equal(dd.cpu().numpy(), disp, equal_nan=True)
    back = lambda t: None if t is None else t.cpu().numpy()
    return (back(vert), back(rgb), back(faces), nv, nf), back(nrm)


def same_image(got, want, what=""):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    bad = (bits(got) != bits(want)).any(axis=2)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def same_list(got, want, what=""):
    """the mesh against mesh_ref's, the normals against the image's rows at the vertices' pixels, the rows behind untouched"""
    mesh, nrm = got
    same_mesh(mesh, want, what)
    V = want["n_vertices"]
    bad = (bits(nrm[:V]) != bits(want["normals"])).any(axis=1)
    assert nrm.dtype == np.float32 and not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:4].tolist())
    assert (nrm[V:] == MARK_F).all(), what


def all_four(e, xyz, disp, col, md, orient, want=None, what=""):
    if want is None:
        want = NR.mesh_grid_normals(xyz, disp, col, md, orient)
    same_image(image_host(e, xyz, disp, md, orient), want["image"], (what, "image host"))
    same_image(image_device(e, xyz, disp, md, orient), want["image"], (what, "image device"))
    same_list(list_host(e, xyz, disp, col, md, orient), want, (what, "list host"))
    same_list(list_device(e, xyz, disp, col, md, orient), want, (what, "list device"))
    return want


# ---- 1. shapes, through all four entries, both orientations ------------------------------------------------------------------------------
@pytest.mark.parametrize("orient", [0, 1])
@pytest.mark.parametrize("i", range(NCASE))
def test_shapes_through_all_four_entries(eng, i, orient):
    H, W, md = MR.SHAPE_CASES[i]
    xyz, disp, col = MR.case_input(i)
    want = NR.case_want(i, orient)
    all_four(eng, xyz, disp, col, md, orient, want, (H, W, orient))
    assert np.array_equal(bits(want["normals"]), bits(want["image"].reshape(-1, 3)[want["pixels"]]))
    # the mesh beside the normals is sgm_mesh_grid's, and without colours too
    same_mesh(list_device(eng, xyz, disp, None, md, orient)[0], MR.case_want(i, False), (H, W, "no colours"))
    a, b = mesh_device(eng, xyz, disp, col, md), list_device(eng, xyz, disp, col, md, orient)[0]
    assert a[3:] == b[3:] and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[:3], b[:3]))
    if i >= 5:
        assert (want["normals"] != 0).any(axis=1).all() and want["n_vertices"] > 20


def test_images_off_a_16_byte_boundary_give_the_same_bits(eng):
    """48 x 320: with an image 4 bytes off a 16-byte boundary k_mesh_quads runs float by float; the normals do not care"""
    import torch
    xyz, disp, col = layered()
    H, W = disp.shape
    n = H * W
    want = NR.mesh_grid_normals(xyz, disp, col, 0.25, 1)
    bx = torch.zeros(n * 3 + 4, dtype=torch.float32, device="cuda")
    bd = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    bo = torch.zeros(n * 3 + 4, dtype=torch.float32, device="cuda")
    assert bx.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0 and bo.data_ptr() % 16 == 0
    for ox, od, oo in ((1, 0, 0), (0, 1, 1), (1, 1, 3), (0, 0, 0)):
        bx[ox:ox + n * 3] = torch.from_numpy(np.array(xyz)).cuda().flatten()
        bd[od:od + n] = torch.from_numpy(np.array(disp)).cuda().flatten()
        bo.fill_(float(MARK_F))
        torch.cuda.synchronize()
        eng.normals_grid_device(bx.data_ptr() + 4 * ox, bd.data_ptr() + 4 * od, H, W, 0.25, 1, bo.data_ptr() + 4 * oo)
        eng.synchronize()
        got = bo.cpu().numpy()
        same_image(got[oo:oo + n * 3].reshape(H, W, 3), want["image"], (ox, od, oo))
        assert (got[:oo] == MARK_F).all() and (got[oo + n * 3:] == MARK_F).all()
        vert = torch.full((n, 3), float(MARK_F), dtype=torch.float32, device="cuda")
        faces = torch.full((2 * (H - 1) * (W - 1), 3), MARK_I, dtype=torch.int32, device="cuda")
        bo.fill_(float(MARK_F))
        torch.cuda.synchronize()
        nv, nf = eng.mesh_grid_normals_device(bx.data_ptr() + 4 * ox, bd.data_ptr() + 4 * od, None, H, W, 0.25, 1, vert.data_ptr(), None,
                                              faces.data_ptr(), bo.data_ptr() + 4 * oo)
        assert (nv, nf) == (want["n_vertices"], want["n_faces"])
        assert np.array_equal(bits(bo.cpu().numpy()[oo:oo + nv * 3].reshape(nv, 3)), bits(want["normals"]))


# ---- 2. extremes at 48 x 320 -----------------------------------------------------------------------------------------------------------
def test_every_pixel_invalid_and_a_checkerboard_give_a_zero_image(eng):
    xyz, disp, col = layered()
    want = all_four(eng, xyz, np.zeros_like(disp), col, 1.0, 1, what="disp 0")
    assert (bits(want["image"]) == 0).all() and want["n_vertices"] == 0
    bx, bd, bc = MR.ramp_cloud(48, 320)
    y, x = np.mgrid[0:48, 0:320]
    bd[(y + x) % 2 == 1] = 0
    want = all_four(eng, bx, bd, bc, 100.0, 1, what="checkerboard")
    assert (bits(want["image"]) == 0).all()


def test_the_ramp_is_0_0_minus_1_everywhere(eng):
    xyz, disp, col = MR.ramp_cloud(48, 320)
    for orient in (0, 1):
        want = all_four(eng, xyz, disp, col, 0.0, orient, what="ramp")
        assert np.array_equal(want["image"], np.broadcast_to(np.array([0, 0, -1], np.float32), (48, 320, 3)))


def test_a_step_edge(eng):
    """left half at Z = 2 and 10 pixels, right half at Z = 3 and 12.5: below the step the two halves are two flat sheets, at it
    the column of quads across the step joins them and the normals of the two columns beside it lean"""
    H, W = 48, 320
    xyz, disp, col = MR.ramp_cloud(H, W, 10.0)
    disp[:, W // 2:] = 12.5
    xyz[:, W // 2:, 2] = 3.0
    flat = np.array([0, 0, -1], np.float32)
    want = all_four(eng, xyz, disp, col, 2.25, 1, what="below the step")
    assert np.array_equal(want["image"], np.broadcast_to(flat, (H, W, 3)))
    want = all_four(eng, xyz, disp, col, 2.5, 1, what="at the step")
    lean = (want["image"] != flat).any(axis=2)
    assert lean[:, W // 2 - 1:W // 2 + 1].all() and not lean[:, :W // 2 - 1].any() and not lean[:, W // 2 + 1:].any()


@pytest.mark.parametrize("md", [0.0, 0.125, 0.25, 1.0, 100.0])
def test_max_diff(eng, md):
    xyz, disp, col = layered()
    want = all_four(eng, xyz, disp, col, md, 1, what=("max_diff", md))
    assert ((want["image"] != 0).any(axis=2).sum() == 0) == (md == 0.0)


def test_the_mixed_orientation_frame(eng):
    xyz, disp, col = NR.mixed_orientation_cloud()
    w0 = all_four(eng, xyz, disp, col, 0.25, 0, what="as wound")
    w1 = all_four(eng, xyz, disp, col, 0.25, 1, what="oriented")
    turned = (w0["normals"] != w1["normals"]).any(axis=1)
    assert turned.sum() >= len(turned) / 4 and (~turned).sum() >= len(turned) / 4
    assert np.array_equal(w0["faces"], w1["faces"])                           # the faces keep their winding


def test_sums_that_overflow_give_zero_and_a_tiny_unit_gives_the_same_bits(eng):
    xyz, disp, col = MR.case_input(6)
    base = NR.case_want(6, 1)
    big = all_four(eng, xyz * F32(2.0 ** 70), disp, col, 0.25, 1, what="2^70")
    kept = (big["normals"] != 0).any(axis=1).mean()
    assert 0.2 < kept < 0.8 and np.isfinite(big["image"]).all()
    small = all_four(eng, xyz * F32(2.0 ** -40), disp, col, 0.25, 1, what="2^-40")
    assert np.array_equal(bits(small["image"]), bits(base["image"]))


def test_the_exact_plane_at_4k_against_its_closed_form():
    """2160 x 3840, every pixel a vertex with the one normal of normals_ref.exact_plane_normal (1 .. 6 triangles, every sum exact):
    the image and the list are that row repeated.  The plane is built on the device and compared there."""
    import torch
    H, W = 2160, 3840
    n, F = H * W, 2 * (H - 1) * (W - 1)
    dev = torch.device("cuda")
    yy = torch.arange(H, device=dev, dtype=torch.float32).view(H, 1).expand(H, W)
    xx = torch.arange(W, device=dev, dtype=torch.float32).view(1, W).expand(H, W)
    dx = torch.stack([xx * 2.0 ** -7, yy * 2.0 ** -7, 2 + xx * 2.0 ** -9 + yy * 2.0 ** -10], dim=2).contiguous()
    small = NR.exact_plane(4, 6)[0]
    assert np.array_equal(dx[:4, :6].cpu().numpy(), small) and np.array_equal(dx[-1, -1].cpu().numpy(), [(W - 1) / 128, (H - 1) / 128, 2 + (W - 1) / 512 + (H - 1) / 1024])
    dd = torch.full((H, W), 8.0, dtype=torch.float32, device=dev)
    row = torch.from_numpy(NR.exact_plane_normal()).to(dev)
    out = torch.full((n, 3), float(MARK_F), dtype=torch.float32, device=dev)
    e = Engine(P16)
    torch.cuda.synchronize()
    e.normals_grid_device(dx.data_ptr(), dd.data_ptr(), H, W, 0.0, 1, out.data_ptr())
    e.synchronize()
    assert torch.equal(out.view(torch.int32), row.view(torch.int32).expand(n, 3))
    vert = torch.empty((n, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
    out.fill_(float(MARK_F))
    torch.cuda.synchronize()
    nv, nf = e.mesh_grid_normals_device(dx.data_ptr(), dd.data_ptr(), None, H, W, 0.0, 0, vert.data_ptr(), None, faces.data_ptr(), out.data_ptr())
    assert (nv, nf) == (n, F) and torch.equal(vert, dx.view(n, 3))
    assert torch.equal(out.view(torch.int32), row.view(torch.int32).expand(n, 3))


# ---- 3. determinism, history, poison, the stage record ---------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bytes(eng):
    xyz, disp, col = layered()
    a, b = list_device(eng, xyz, disp, col, 0.25, 1), list_device(eng, xyz, disp, col, 0.25, 1)
    assert a[0][3:] == b[0][3:] and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))
    assert np.array_equal(bits(image_device(eng, xyz, disp, 0.25, 1)), bits(image_device(eng, xyz, disp, 0.25, 1)))
    same_list(a, NR.mesh_grid_normals(xyz, disp, col, 0.25, 1))


def test_results_do_not_depend_on_what_the_engine_did_before():
    e = Engine(P16)

    def run(i, listfn, imagefn):
        xyz, disp, col = MR.case_input(i)
        md = MR.SHAPE_CASES[i][2]
        same_list(listfn(e, xyz, disp, col, md, 1), NR.case_want(i, 1), (i, listfn.__name__))
        same_image(imagefn(e, xyz, disp, md, 0), NR.case_want(i, 0)["image"], (i, imagefn.__name__))
    big, small = 7, 5                       # 97 x 331, then 3 x 257
    run(small, list_host, image_host)
    run(big, list_device, image_device)
    run(small, list_device, image_device)   # a smaller frame in the larger maps
    run(big, list_host, image_host)
    e.trim()                                # gives the maps and the staged normals back; they return on the next call
    run(small, list_device, image_host)
    try:
        for byte in (0xA5, 0x7F, 0x00, 0xFF):
            e.set_option(_lib.SGM_OPT_POISON, byte)      # fills every buffer the engine owns and arms the same for new ones
            run(small, list_host, image_device)
            e.set_option(_lib.SGM_OPT_POISON, byte)
            run(big, list_device, image_host)
            e.set_option(_lib.SGM_OPT_POISON, byte)
            xyz, disp, _ = MR.case_input(small)          # the image alone on poisoned maps: no vertex numbers exist
            same_image(image_device(e, xyz, disp, MR.SHAPE_CASES[small][2], 1), NR.case_want(small, 1)["image"], byte)
    finally:
        e.set_option(_lib.SGM_OPT_POISON, -1)


def test_the_profile_record_names_the_stages():
    e = Engine(P16)
    xyz, disp, col = layered()
    want = NR.mesh_grid_normals(xyz, disp, col, 0.25, 1)
    try:
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        same_list(list_device(e, xyz, disp, col, 0.25, 1), want)
        st = {n: launches for n, ms, launches in e.stage_times()}
        assert st == dict(STAGES, mesh_normals=1) and list(st)[-2:] == ["mesh_normals", "_wall"], st
        same_image(image_device(e, xyz, disp, 0.25, 1), want["image"])
        st = {n: launches for n, ms, launches in e.stage_times()}
        assert st == {"mesh_quads": 1, "normals_grid": 1, "_wall": 0}, st
        same_mesh(mesh_device(e, xyz, disp, col, 0.25), want)                  # ... and sgm_mesh_grid's own record is what it was
        assert {n: launches for n, ms, launches in e.stage_times()} == STAGES
    finally:
        e.set_option(_lib.SGM_OPT_PROFILE, 0)


# ---- 4. the existing paths ---------------------------------------------------------------------------------------------------------------
def test_the_mesh_the_compaction_and_the_voxel_grid_are_unchanged_after_a_normals_call():
    e = Engine(P16)
    xyz, disp, col = MR.layered_cloud(97, 331, 9)
    mask = ~np.isnan(xyz[:, :, 0]) & ~np.isinf(xyz[:, :, 0]) & (disp > 0)
    lst = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)
    vox = VR.voxel_downsample(*lst, 0.05)
    mesh = MR.mesh_grid(xyz, disp, col, 0.25)

    def existing(when):
        same_mesh(mesh_host(e, xyz, disp, col, 0.25), mesh, when)
        same_mesh(mesh_device(e, xyz, disp, col, 0.25), mesh, when)
        p, c = e.compact_points_host(xyz, disp, col)
        assert np.array_equal(p.view(np.uint32), xyz[mask].view(np.uint32)) and np.array_equal(c, col[mask]), when
        p, c, k, noor = e.voxel_downsample_host(*lst, 0.05, return_counts=True)
        assert noor == vox["n_out_of_range"] and np.array_equal(p.view(np.uint32), vox["points"].view(np.uint32)), when
        assert np.array_equal(c, vox["colors"]) and np.array_equal(k, vox["counts"]), when
    existing("before")
    all_four(e, xyz, disp, col, 1.0, 1)
    existing("after")
    all_four(e, xyz[:40, :100], disp[:40, :100], col[:40, :100], 0.25, 0)
    existing("after a smaller frame")


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched_and_the_engine_usable(eng):
    L = _lib.load()
    xyz, disp, col = (np.array(a[:10, :10]) for a in layered())
    H = W = 10
    vert, nrm = np.full((100, 3), MARK_F, np.float32), np.full((100, 3), MARK_F, np.float32)
    rgb, faces = np.full((100, 3), MARK_B, np.uint8), np.full((162, 3), MARK_I, np.int32)
    nv, nf = C.c_int64(-5), C.c_int64(-6)
    X, D, Cc, P, R, Fp, Np = (a.ctypes.data for a in (xyz, disp, col, vert, rgb, faces, nrm))
    NV, NF = C.byref(nv), C.byref(nf)
    h = eng._h
    good = (h, X, D, Cc, H, W, 1.0, 1, P, R, Fp, Np, NV, NF)

    def but(args, **kw):
        """the good call with some arguments replaced, by name"""
        names = ("e", "xyz", "disp", "col", "H", "W", "md", "orient", "vert", "rgb", "faces", "nrm", "nv", "nf") if len(args) == 14 else \
            ("e", "xyz", "disp", "H", "W", "md", "orient", "nrm")
        assert set(kw) <= set(names)
        return tuple(kw.get(k, v) for k, v in zip(names, args))
    bad = [dict(e=None), dict(xyz=None), dict(disp=None), dict(vert=None), dict(faces=None), dict(nrm=None), dict(nv=None), dict(nf=None),
           dict(H=0), dict(W=0), dict(H=-3), dict(md=-1.0), dict(md=float("nan")), dict(md=float("inf")), dict(md=-1e-30),
           dict(col=None), dict(orient=2), dict(orient=-1), dict(orient=256)]
    for fn in (L.sgm_mesh_grid_normals, L.sgm_mesh_grid_normals_device):
        for kw in bad:
            assert fn(*but(good, **kw)) == -1, kw                                   # SGM_ERR_INVALID_ARG
            assert b"sgm_mesh_grid_normals" in L.sgm_last_error()
        assert fn(*but(good, H=8193, W=8192)) == -4 and b"2^26" in L.sgm_last_error()      # SGM_ERR_UNSUPPORTED: before anything is read
    good_img = (h, X, D, H, W, 1.0, 1, Np)
    for fn in (L.sgm_normals_grid, L.sgm_normals_grid_device):
        for kw in bad:
            if set(kw) & {"vert", "faces", "nv", "nf", "col"}:
                continue
            assert fn(*but(good_img, **kw)) == -1, kw
            assert b"sgm_normals_grid" in L.sgm_last_error()
        assert fn(*but(good_img, H=8193, W=8192)) == -4 and b"2^26" in L.sgm_last_error()
    assert (vert == MARK_F).all() and (nrm == MARK_F).all() and (rgb == MARK_B).all() and (faces == MARK_I).all()
    assert (nv.value, nf.value) == (-5, -6)
    # no quad: the list entries succeed with 0 and 0 and write nothing, the image entries write a zero image of the frame's size
    for fn in (L.sgm_mesh_grid_normals, L.sgm_mesh_grid_normals_device):
        for hh, ww in ((1, 100), (100, 1), (1, 1)):
            nv.value, nf.value = -5, -6
            assert fn(*but(good, col=None, rgb=None, H=hh, W=ww)) == 0 and (nv.value, nf.value) == (0, 0)
    assert (vert == MARK_F).all() and (nrm == MARK_F).all() and (faces == MARK_I).all()
    for hh, ww in ((1, 30), (30, 1), (1, 1)):
        assert L.sgm_normals_grid(*but(good_img, H=hh, W=ww)) == 0
        assert (bits(nrm[:hh * ww]) == 0).all() and (nrm[hh * ww:] == MARK_F).all()
        nrm[:] = MARK_F
        got = image_device(eng, np.ones((hh, ww, 3), np.float32), np.ones((hh, ww), np.float32), 1.0, 1)
        assert (bits(got) == 0).all()
    all_four(eng, *layered(), 0.25, 1, what="after the refusals")


# ---- 6. the Python surface, on a frame of the size users run ----------------------------------------------------------------------------------
def test_the_python_surface_on_a_1080p_frame_from_the_pipeline(tmp_path):
    """1080 x 1920 through StereoSGBM and reprojectImageTo3D, then estimate_normals and triangulate_points_with_normals on the
    default engine, with and without a confidence mask, and out to a file and back"""
    H, W, D = 1080, 1920, 128
    a, b = synth.make_pair(H, W, D, seed=5)[:2]
    e = Engine(U.params(D, 5, 0, 1))
    disp = e.disp_to_float_host(e.compute_host(a, b))
    xyz = sgm.reprojectImageTo3D(disp, synth.default_Q(W))
    col = np.repeat(a[:, :, None], 3, axis=2) ^ np.array([0, 85, 170], np.uint8)
    assert MR.valid_mask(xyz, disp).mean() > 0.3
    want = NR.mesh_grid_normals(xyz, disp, col, 1.0, 1)
    img = sgm.estimate_normals(xyz, disp)                                   # max_diff = 1.0 and orient = True are the defaults
    assert img.dtype == np.float32 and img.shape == (H, W, 3)
    same_image(img, want["image"], "estimate_normals")
    v, c, t, n = sgm.triangulate_points_with_normals(xyz, col, disp)
    assert n.dtype == np.float32 and t.shape[0] > 100000 and np.array_equal(bits(n), bits(want["normals"]))
    assert np.array_equal(bits(v), bits(want["vertices"])) and np.array_equal(c, want["colors"]) and np.array_equal(t, want["faces"])
    v3, c3, t3 = sgm.triangulate_points(xyz, col, disp)
    assert np.array_equal(bits(v3), bits(v)) and np.array_equal(c3, c) and np.array_equal(t3, t)
    with np.errstate(all="ignore"):
        towards = (n.astype(np.float64) * v.astype(np.float64)).sum(axis=1)
    assert (towards <= 1e-6 * np.abs(v).max()).all() and (n != 0).any(axis=1).mean() > 0.999
    # unoriented, at another max_diff, on a crop: the reference is cheap there
    crop = np.s_[300:420, 700:1000]
    w2 = NR.mesh_grid_normals(xyz[crop], disp[crop], None, 0.5, 0)
    same_image(sgm.estimate_normals(xyz[crop], disp[crop], 0.5, orient=False), w2["image"], "crop")
    conf = np.random.default_rng(3).integers(0, 101, size=disp[crop].shape).astype(np.uint8)
    w3 = NR.mesh_grid_normals(xyz[crop], np.where(conf >= 40, disp[crop], F32(0)), None, 1.0, 1)
    v, c, t, n = sgm.triangulate_points_with_normals(xyz[crop], None, disp[crop], confidence=conf, min_confidence=40)
    assert c is None and 0 < w3["n_faces"] and np.array_equal(t, w3["faces"]) and np.array_equal(bits(n), bits(w3["normals"]))
    same_image(sgm.estimate_normals(xyz[crop], disp[crop], confidence=conf, min_confidence=40), w3["image"], "confidence")
    path = str(tmp_path / "m.ply")
    sgm.write_ply(path, v, None, n, t)
    rp, rc, rn, rt = sgm.read_ply(path)
    assert np.array_equal(rp, v.astype(np.float64)) and rc is None and np.array_equal(rn, n.astype(np.float64)) and np.array_equal(rt, t)


# ---- 7. guarded buffers -------------------------------------------------------------------------------------------------------------------
def test_the_cases_with_every_buffer_guarded():
    """(the same cases ran in the plain mode above)"""
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "normals_guard_child.py")], capture_output=True, text=True, env=env,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"NORMALS_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) >= 12, tail
