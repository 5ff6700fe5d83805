"""The edge-aware disparity filter on the device (needs an MI355X): sgm_wls_filter, sgm_wls_filter_device,
createDisparityWLSFilter, StereoSGBM.computeFiltered.

Yardstick: tests/wls_ref.py in float32 -- the definition of include/sgm_hip_wls.h, one numpy ufunc per operation;
tests/test_wls_reference.py ties it to answers worked out by hand.  Every comparison is bit for bit: the int16 map, and the
float map through its bit pattern."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bruteforce_color as BC
import parity_util as U
import wls_ref as WR
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd import stereo as cv
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = dict(numDisparities=16)


@functools.lru_cache(maxsize=None)
def _weights(sigma):
    return WR.weights(sigma)


@functools.lru_cache(maxsize=None)
def _case(H, W, cn, with_conf, lam, sigma, invalid, seed=0, holes=0.3):
    """(input, reference), computed once per case and shared; nobody writes to either"""
    s = WR.random_input(H, W, cn, seed, invalid, holes, with_conf)
    want = WR.wls_filter(s["disp"], s["guide"], s["conf"], invalid, lam, _weights(sigma))
    for a in list(s.values()) + list(want.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return s, want


def _same(out, outf, want, what=""):
    assert out.dtype == np.int16 and np.array_equal(out, want["out"]), (what, int((out != want["out"]).sum()))
    if outf is not None:
        assert outf.dtype == np.float32
        nbad = int((outf.view(np.uint32) != want["out_f32"].view(np.uint32)).sum())
        assert nbad == 0, (what, nbad)


@pytest.fixture(scope="module")
def eng():
    return Engine(P16)


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,cn,with_conf,lam,sigma,invalid", WR.SHAPE_CASES)
def test_shapes_through_the_host_entry(eng, H, W, cn, with_conf, lam, sigma, invalid):
    s, want = _case(H, W, cn, with_conf, lam, sigma, invalid)
    out, outf = eng.wls_filter_host(s["disp"], s["guide"], s["conf"], invalid, lam, _weights(sigma), return_float=True)
    _same(out, outf, want, (H, W, cn))
    if H * W > 100:
        assert 0 < want["valid"].sum() and (want["out"] != s["disp"]).any()     # the case does something


# Every shape of the line kernels gives the same bits (csrc/sgm_debug.h): the five of wls_rows_shapes beside the default column
# shape, the four of wls_cols_shapes beside the default row shape.  A single map is a chunk of one, so a shape picked for such
# chunks is what every single call runs; a non-zero field selects its shape for every chunk, 0 leaves the choice to the library
# (one pair of shapes for the single calls below, another for the batches of three).
ROWS_SHIFT, COLS_SHIFT = 17, 20       # SGM_DBG_WLS_BATCH_ROWS_SHIFT, SGM_DBG_WLS_BATCH_COLS_SHIFT
LINE_SHAPES = [("rows", i, i << ROWS_SHIFT) for i in range(5)] + [("cols", i, i << COLS_SHIFT) for i in range(4)]


@pytest.mark.parametrize("debug", [d for _, _, d in LINE_SHAPES], ids=[f"{k}{i}" for k, i, _ in LINE_SHAPES])
def test_every_line_kernel_shape_gives_the_same_bits(debug):
    import torch
    e = Engine(P16)
    e.set_option(_lib.SGM_OPT_DEBUG, debug)
    dev = torch.device("cuda", e.device)
    up = lambda a: None if a is None else torch.from_numpy(a.copy()).to(dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    for case in WR.SHAPE_CASES:
        H, W, cn, with_conf, lam, sigma, invalid = case
        s, want = _case(*case)
        d, g, c = up(s["disp"]), up(s["guide"]), up(s["conf"])
        out = torch.full((H, W), 77, dtype=torch.int16, device=dev)
        outf = torch.full((H, W), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        e.wls_filter_device(ptr(d), ptr(g), cn, ptr(c), H, W, invalid, lam, _weights(sigma), ptr(out), ptr(outf))
        e.synchronize()
        _same(out.cpu().numpy(), outf.cpu().numpy(), want, ("single", debug, H, W, cn))
    for case in (WR.SHAPE_CASES[6], WR.SHAPE_CASES[7]):       # 65 x 129 gray with confidence, 130 x 67 colour without
        H, W, cn, with_conf, lam, sigma, invalid = case
        maps = [_case(*case, seed=2000 + i) for i in range(3)]
        d, g, c = ([up(s[k]) for s, _ in maps] for k in ("disp", "guide", "conf"))
        out = [torch.full((H, W), 77, dtype=torch.int16, device=dev) for _ in maps]
        outf = [torch.full((H, W), 7.0, dtype=torch.float32, device=dev) for _ in maps]
        ptrs = lambda ts: None if ts[0] is None else [t.data_ptr() for t in ts]
        torch.cuda.synchronize()
        e.wls_filter_batch_device(ptrs(d), ptrs(g), cn, ptrs(c), H, W, invalid, lam, _weights(sigma), ptrs(out), ptrs(outf))
        e.synchronize()
        for i, (_, want) in enumerate(maps):
            _same(out[i].cpu().numpy(), outf[i].cpu().numpy(), want, ("batch", debug, H, W, cn, i))


# ---- 2. lambda / sigma, channels, confidence ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam,sigma", [(0.0, 1.5), (100.0, 10.0), (8000.0, 1.5), (8000.0, 0.5), (1e6, 1.5)])
@pytest.mark.parametrize("H,W,cn,with_conf,invalid", [(65, 129, 1, False, -160), (130, 67, 3, True, -16)])
def test_lambda_and_sigma(eng, H, W, cn, with_conf, invalid, lam, sigma):
    s, want = _case(H, W, cn, with_conf, lam, sigma, invalid, seed=5)
    out, outf = eng.wls_filter_host(s["disp"], s["guide"], s["conf"], invalid, lam, _weights(sigma), return_float=True)
    _same(out, outf, want, (H, W, cn, lam, sigma))


@pytest.mark.parametrize("cn", [1, 3])
def test_all_invalid_and_all_valid_maps(eng, cn):
    s, want = _case(65, 129, cn, True, 8000.0, 1.5, -16, seed=6, holes=2.0)
    assert (s["disp"] == -16).all()
    out, outf = eng.wls_filter_host(s["disp"], s["guide"], s["conf"], -16, 8000.0, _weights(1.5), return_float=True)
    assert (out == -16).all() and (outf.view(np.uint32) == 0).all()
    _same(out, outf, want)
    s, want = _case(65, 129, cn, cn == 1, 8000.0, 1.5, -16, seed=6, holes=-1.0)
    assert (s["disp"] != -16).all()
    out, outf = eng.wls_filter_host(s["disp"], s["guide"], s["conf"], -16, 8000.0, _weights(1.5), return_float=True)
    _same(out, outf, want)
    if cn == 3:
        assert (out != -16).all()       # full confidence everywhere: every pixel stays valid


def test_hand_made_tables(eng):
    """the table is an input: all ones (the guide does not matter), and a hard edge (weights of exactly zero above index 8 cut
    the lines into independent pieces)"""
    s, _ = _case(97, 260, 3, True, 8000.0, 1.5, -16, seed=7)
    ones = np.ones(256, np.float32)
    hard = (np.arange(256) <= 8).astype(np.float32)
    for lut in (ones, hard):
        want = WR.wls_filter(s["disp"], s["guide"], s["conf"], -16, 8000.0, lut)
        out, outf = eng.wls_filter_host(s["disp"], s["guide"], s["conf"], -16, 8000.0, lut, return_float=True)
        _same(out, outf, want)
    flat = eng.wls_filter_host(s["disp"], np.zeros_like(s["guide"]), s["conf"], -16, 8000.0, ones)
    assert np.array_equal(flat, eng.wls_filter_host(s["disp"], s["guide"], s["conf"], -16, 8000.0, ones))


# ---- 3. entry points --------------------------------------------------------------------------------------------------------------
def test_device_entry_aliasing_and_no_float_map(eng):
    import torch
    dev = torch.device("cuda", eng.device)
    for (H, W, cn, with_conf, lam, sigma, invalid) in (WR.SHAPE_CASES[6], WR.SHAPE_CASES[7]):
        s, want = _case(H, W, cn, with_conf, lam, sigma, invalid)
        d = torch.from_numpy(s["disp"].copy()).to(dev)
        g = torch.from_numpy(s["guide"].copy()).to(dev)
        c = None if s["conf"] is None else torch.from_numpy(s["conf"].copy()).to(dev)
        out = torch.full((H, W), 77, dtype=torch.int16, device=dev)
        outf = torch.full((H, W), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        cp = None if c is None else c.data_ptr()
        eng.wls_filter_device(d.data_ptr(), g.data_ptr(), cn, cp, H, W, invalid, lam, _weights(sigma), out.data_ptr(), outf.data_ptr())
        eng.synchronize()
        _same(out.cpu().numpy(), outf.cpu().numpy(), want, "device entry")
        assert np.array_equal(d.cpu().numpy(), s["disp"]) and np.array_equal(g.cpu().numpy(), s["guide"])   # inputs untouched
        # out_f32 null, and out == disp
        eng.wls_filter_device(d.data_ptr(), g.data_ptr(), cn, cp, H, W, invalid, lam, _weights(sigma), d.data_ptr(), None)
        eng.synchronize()
        _same(d.cpu().numpy(), None, want, "in place")
    # the host entry: out is disp, no float map
    s, want = _case(*WR.SHAPE_CASES[6])
    buf = s["disp"].copy()
    lut = _weights(1.5)
    L = _lib.load()
    rc = L.sgm_wls_filter(eng._h, buf.ctypes.data, s["guide"].ctypes.data, 1, s["conf"].ctypes.data, 65, 129, -16, C.c_double(8000.0),
                          lut.ctypes.data, buf.ctypes.data, None)
    assert rc == 0, _lib.last_error()
    _same(buf, None, want, "host in place")


def test_tensors_in_tensors_out():
    import torch
    H, W, cn, with_conf, lam, sigma, invalid = WR.SHAPE_CASES[9]
    s, want = _case(H, W, cn, with_conf, lam, sigma, invalid)
    f = cv.createDisparityWLSFilter()
    f.setLambda(lam)
    f.setSigmaColor(sigma)
    t = lambda a: torch.from_numpy(a.copy()).cuda()
    out, outf = f.filter(t(s["disp"]), t(s["guide"]), t(s["conf"]), return_float=True)
    assert out.is_cuda and outf.is_cuda and out.dtype == torch.int16 and outf.dtype == torch.float32
    _same(out.cpu().numpy(), outf.cpu().numpy(), want, "tensors")
    got = f.filter(s["disp"], s["guide"], s["conf"])
    assert isinstance(got, np.ndarray)
    _same(got, None, want, "numpy")
    with pytest.raises(cv.error, match="CUDA"):
        f.filter(t(s["disp"]), s["guide"])
    # the default invalid value comes from the matcher
    s2, want2 = _case(*WR.SHAPE_CASES[8])
    f2 = cv.createDisparityWLSFilter(cv.StereoSGBM_create(minDisparity=-9, numDisparities=16))
    f2.setSigmaColor(0.5)
    _same(f2.filter(s2["disp"], s2["guide"], s2["conf"]), None, want2, "matcher's invalid")


# ---- 4. history -------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_the_engine_did_before():
    p = U.params(64, 5, 0, 1)
    l, r, _ = synth.make_pair(48, 320, 64, 7)
    big, small = WR.SHAPE_CASES[6], WR.SHAPE_CASES[4]
    e = Engine(p)
    run = lambda case: e.wls_filter_host(_case(*case)[0]["disp"], _case(*case)[0]["guide"], _case(*case)[0]["conf"], case[6], case[4],
                                         _weights(case[5]), return_float=True)
    a1 = run(big)
    c1 = e.compute_host(l, r)
    b = run(small)
    a2 = run(big)
    c2 = e.compute_host(l, r)
    _same(*a1, _case(*big)[1])
    _same(*b, _case(*small)[1])
    _same(*a2, _case(*big)[1])
    e.trim()                                  # gives the planes back; they return on the next call
    _same(*run(big), _case(*big)[1])
    fresh = Engine(p).compute_host(l, r)
    assert np.array_equal(c1, fresh) and np.array_equal(c2, fresh)


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(eng):
    import torch
    L = _lib.load()
    s, want = _case(*WR.SHAPE_CASES[6])
    H, W = 65, 129
    lut = _weights(1.5)
    out = np.full((H, W), 77, np.int16)
    dev = torch.device("cuda", eng.device)
    dd, dg, dc = (torch.from_numpy(s[k].copy()).to(dev) for k in ("disp", "guide", "conf"))
    dout = torch.full((H, W), 77, dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    good = dict(e=eng._h, disp=s["disp"].ctypes.data, guide=s["guide"].ctypes.data, cn=1, conf=s["conf"].ctypes.data, H=H, W=W, invalid=-16,
                lam=8000.0, lut=lut.ctypes.data, out=out.ctypes.data, outf=None)
    good_d = dict(good, disp=dd.data_ptr(), guide=dg.data_ptr(), conf=dc.data_ptr(), out=dout.data_ptr())
    bad = [dict(disp=None), dict(guide=None), dict(lut=None), dict(out=None), dict(e=None), dict(H=0), dict(W=0), dict(H=-3), dict(W=-1),
           dict(cn=2), dict(cn=0), dict(cn=4), dict(lam=-1.0), dict(lam=1e7 + 1), dict(lam=float("nan")), dict(lam=float("inf")),
           dict(invalid=32768), dict(invalid=-32769)]
    call = lambda fn, a: fn(a["e"], a["disp"], a["guide"], a["cn"], a["conf"], a["H"], a["W"], a["invalid"], C.c_double(a["lam"]), a["lut"],
                            a["out"], a["outf"])
    for fn, base in ((L.sgm_wls_filter, good), (L.sgm_wls_filter_device, good_d)):
        for b in bad:
            assert call(fn, dict(base, **b)) == -1, b                 # SGM_ERR_INVALID_ARG
            assert b"sgm_wls_filter" in L.sgm_last_error()
    eng.synchronize()
    assert (out == 77).all() and (dout.cpu().numpy() == 77).all()     # nothing was enqueued
    assert call(L.sgm_wls_filter, good) == 0
    _same(out, None, want)
    assert call(L.sgm_wls_filter_device, good_d) == 0
    eng.synchronize()
    _same(dout.cpu().numpy(), None, want)


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------
def test_compute_filtered_is_the_filter_behind_compute_with_confidence():
    import torch
    lut = _weights(1.5)
    l, r, _ = synth.make_pair(48, 320, 64, 7)
    L3, R3 = BC.colour_pair(40, 200, 32, seed=22)
    for left, right, p in ((l, r, U.params(64, 5, 0, 1)), (L3, R3, U.params(32, 3, 0, 1, penalty="plain"))):
        m = cv.StereoSGBM_create(**p)
        before = m.compute(left, right)
        got = m.computeFiltered(left, right)
        disp, conf = m.computeWithConfidence(left, right)
        assert np.array_equal(disp, before)
        want = WR.wls_filter(disp, left, conf, -16, 8000.0, lut)
        _same(got, None, want, "computeFiltered")
        assert (got != before).any()       # (bit parity, not quality: this texture has no edges at its depth steps)
        t = m.computeFiltered(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda())
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), got)
        other = m.computeFiltered(left, right, lambda_=500.0, sigmaColor=3.0)
        _same(other, None, WR.wls_filter(disp, left, conf, -16, 500.0, _weights(3.0)), "computeFiltered, other settings")
        assert np.array_equal(m.compute(left, right), before)


# ---- 7. guarded buffers -----------------------------------------------------------------------------------------------------------
def test_shapes_with_every_buffer_guarded():
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wls_guard_child.py")], capture_output=True, text=True,
                       env=env, timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"WLS_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) == len(WR.SHAPE_CASES), tail
