"""The left-right consistency confidence on the device (needs an MI355X): sgm_lrc_confidence, sgm_lrc_confidence_device,
sgm_lrc_confidence_batch_device, lrcConfidence, DisparityWLSFilter.filter / filterBatch with a right-view map, getConfidenceMap,
StereoSGBM.computeFiltered / computeFilteredBatch with confidence="lrc" / "both".

Yardstick: tests/lrc_ref.py -- the definition of include/sgm_hip_lrc.h in numpy, windows formed directly -- bit for bit.  The
shape list is LR.SHAPE_CASES (which says what straddles the kernels' tiles); every pair of a batch has a seed of its own, so a
mixed-up pair index shows.  Where the filter follows, the yardstick is the filter fed with the reference confidence."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bruteforce_color as BC
import lrc_ref as LR
import parity_util as U
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd import stereo as cv
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = dict(numDisparities=16)
NCASE = len(LR.SHAPE_CASES)


@pytest.fixture(scope="module")
def eng():
    return Engine(P16)


@functools.lru_cache(maxsize=None)
def _pair(H, W, seed, invalid, r, T, V, with_base=True, levels=None):
    """(input, (conf_left, conf_right)) of ONE pair, computed once and shared; nobody writes to either"""
    s = LR.random_pair(H, W, seed, invalid, levels)
    want = LR.lrc_confidence(s["dl"], s["dr"], s["base"] if with_base else None, invalid, T, r, V)
    for a in list(s.values()) + list(want):
        a.setflags(write=False)
    return s, want


def _device(e, ins, with_base, invalid, T, r, V, left=True, right=True, batch=True):
    """every map in a tensor of its own; the outputs pre-filled with a marker; the inputs checked untouched"""
    import torch
    dev = torch.device("cuda", e.device)
    H, W = ins[0]["dl"].shape
    up = lambda key: [torch.from_numpy(s[key].copy()).to(dev) for s in ins]
    dl, dr, b = up("dl"), up("dr"), up("base") if with_base else None
    cl = [torch.full((H, W), 177, dtype=torch.uint8, device=dev) for _ in ins] if left else None
    cr = [torch.full((H, W), 177, dtype=torch.uint8, device=dev) for _ in ins] if right else None
    ptrs = lambda ts: None if ts is None else [x.data_ptr() for x in ts]
    torch.cuda.synchronize()
    if batch:
        e.lrc_confidence_batch_device(ptrs(dl), ptrs(dr), ptrs(b), H, W, invalid, T, r, V, ptrs(cl), ptrs(cr))
    else:
        for i in range(len(ins)):
            e.lrc_confidence_device(dl[i].data_ptr(), dr[i].data_ptr(), None if b is None else b[i].data_ptr(), H, W, invalid, T, r, V,
                                    None if cl is None else cl[i].data_ptr(), None if cr is None else cr[i].data_ptr())
    e.synchronize()
    for i, s in enumerate(ins):
        assert np.array_equal(dl[i].cpu().numpy(), s["dl"]) and np.array_equal(dr[i].cpu().numpy(), s["dr"])
        assert b is None or np.array_equal(b[i].cpu().numpy(), s["base"])
    back = lambda ts: None if ts is None else [x.cpu().numpy() for x in ts]
    return back(cl), back(cr)


def _same(got, want, what=""):
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (what, int((got != want).sum()))


# ---- 1. shapes, through the three entries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NCASE))
def test_shapes_through_every_entry(eng, i):
    H, W, r, T, V, invalid, levels = LR.SHAPE_CASES[i]
    s = LR.case_input(i)
    for with_base in (True, False):
        wl, wr = LR.case_want(i, with_base)
        b = s["base"] if with_base else None
        cl, cr = eng.lrc_confidence_host(s["dl"], s["dr"], b, invalid, T, r, V, True, True)
        _same(cl, wl, ("host left", with_base))
        _same(cr, wr, ("host right", with_base))
        for batch in (False, True):
            cl, cr = _device(eng, [s], with_base, invalid, T, r, V, batch=batch)
            _same(cl[0], wl, ("device left", with_base, batch))
            _same(cr[0], wr, ("device right", with_base, batch))
    # either output alone
    wl, wr = LR.case_want(i, True)
    cl, cr = eng.lrc_confidence_host(s["dl"], s["dr"], s["base"], invalid, T, r, V, True, False)
    assert cr is None
    _same(cl, wl, "left alone")
    cl, cr = eng.lrc_confidence_host(s["dl"], s["dr"], s["base"], invalid, T, r, V, False, True)
    assert cl is None
    _same(cr, wr, "right alone")
    cl, cr = _device(eng, [s], True, invalid, T, r, V, left=False)
    assert cl is None
    _same(cr[0], wr, "device, right alone")
    cl, cr = _device(eng, [s], True, invalid, T, r, V, right=False, batch=False)
    assert cr is None
    _same(cl[0], wl, "device, left alone")


def test_all_invalid_all_valid_and_the_extreme_maps(eng):
    H, W = 65, 129
    s = dict(_pair(H, W, 7, -16, 5, 24, 2304)[0])
    gone = np.full((H, W), -16, np.int16)
    for dl, dr in ((gone, s["dr"]), (s["dl"], gone), (gone, gone)):
        cl, cr = eng.lrc_confidence_host(dl, dr, s["base"], -16, 24, 5, 2304, True, True)
        assert (cl == 0).all() and (cr == 0).all()
    full = LR.random_pair(H, W, 8, -16, holes=-1.0)                         # no holes: every pixel valid
    assert (full["dl"] != -16).all()
    want = LR.lrc_confidence(full["dl"], full["dr"], full["base"], -16, 24, 5, 2304)
    got = eng.lrc_confidence_host(full["dl"], full["dr"], full["base"], -16, 24, 5, 2304, True, True)
    _same(got[0], want[0]), _same(got[1], want[1])
    # maps alternating -32768 / 32767 at r = 16: the largest sums, at both ends of var_max, and through the batch entry
    x = LR.extreme_pair(40, 70)
    for V, T in ((1, 32767), (1 << 30, 32767), (1 << 30, 0), (2304, 24)):
        want = LR.lrc_confidence(x["dl"], x["dr"], x["base"], -16, T, 16, V)
        got = eng.lrc_confidence_host(x["dl"], x["dr"], x["base"], -16, T, 16, V, True, True)
        _same(got[0], want[0], ("extreme left", V, T)), _same(got[1], want[1], ("extreme right", V, T))
    # ... and a pair where the extremes MATCH (the right map the left one shifted by nothing: d = 32767 leaves the image, -32768 too)
    flat = dict(dl=np.full((40, 70), 32767, np.int16), dr=np.full((40, 70), 32767, np.int16), base=x["base"])
    flat["dl"][:, ::3] = 5
    flat["dr"][:, ::3] = 9
    want = LR.lrc_confidence(flat["dl"], flat["dr"], None, -16, 24, 16, 1 << 30)
    assert want[0].max() > 0
    got = _device(eng, [flat], False, -16, 24, 16, 1 << 30)
    _same(got[0][0], want[0]), _same(got[1][0], want[1])


# ---- 2. batches and chunks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,r,invalid", [(1, 65, 129, 6, -16), (2, 33, 97, 16, -160), (5, 64, 64, 4, -16), (3, 17, 257, 3, -16)])
def test_batches_equal_the_reference_and_single_calls(eng, N, H, W, r, invalid):
    pairs = [_pair(H, W, 900 + 10 * N + k, invalid, r, 24, 2304) for k in range(N)]
    ins, wants = [p[0] for p in pairs], [p[1] for p in pairs]
    assert N == 1 or not np.array_equal(wants[0][0], wants[1][0])
    cl, cr = _device(eng, ins, True, invalid, 24, r, 2304)
    sl, sr = _device(eng, ins, True, invalid, 24, r, 2304, batch=False)
    for k in range(N):
        _same(cl[k], wants[k][0], ("batch left", k)), _same(cr[k], wants[k][1], ("batch right", k))
        _same(sl[k], wants[k][0], ("single left", k)), _same(sr[k], wants[k][1], ("single right", k))


def test_chunks_give_the_same_results():
    """N = 5 in chunks of 2 + 2 + 1 and of 1 x 5 (SGM_OPT_GROUP_MAX) against one chunk; N = 66 at a small shape is above the
    largest chunk (64) whatever the option says"""
    e = Engine(P16)
    pairs = [_pair(65, 129, 300 + k, -160, 6, 24, 2304) for k in range(5)]
    ins, wants = [p[0] for p in pairs], [p[1] for p in pairs]
    try:
        for gm in (0, 2, 1, 0):
            e.set_option(_lib.SGM_OPT_GROUP_MAX, gm)
            cl, cr = _device(e, ins, True, -160, 24, 6, 2304)
            for k in range(5):
                _same(cl[k], wants[k][0], ("left, group_max", gm, k)), _same(cr[k], wants[k][1], ("right, group_max", gm, k))
    finally:
        e.set_option(_lib.SGM_OPT_GROUP_MAX, 0)
    pairs = [_pair(9, 40, 400 + k, -16, 3, 24, 2304) for k in range(66)]
    ins, wants = [p[0] for p in pairs], [p[1] for p in pairs]
    cl, cr = _device(e, ins, False, -16, 24, 3, 2304)
    for k in range(66):
        w = LR.lrc_confidence(ins[k]["dl"], ins[k]["dr"], None, -16, 24, 3, 2304)
        _same(cl[k], w[0], ("N = 66, left", k)), _same(cr[k], w[1], ("N = 66, right", k))


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(eng):
    import torch
    L = _lib.load()
    N, H, W, r = 3, 33, 97, 5
    pairs = [_pair(H, W, 700 + k, -16, r, 24, 2304) for k in range(N)]
    ins, wants = [p[0] for p in pairs], [p[1] for p in pairs]
    dev = torch.device("cuda", eng.device)
    up = lambda key: torch.from_numpy(np.stack([s[key] for s in ins])).to(dev)
    dl, dr, b = up("dl"), up("dr"), up("base")
    cl = torch.full((N, H, W), 177, dtype=torch.uint8, device=dev)
    cr = torch.full((N, H, W), 177, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    arr = lambda t, hole=None: (C.c_void_p * N)(*[None if i == hole else t[i].data_ptr() for i in range(N)])
    mixed = lambda t, i, other: (C.c_void_p * N)(*[other.data_ptr() if k == i else t[k].data_ptr() for k in range(N)])
    # the host entry and the single device entry: one signature
    h = ins[0]
    hcl, hcr = np.full((H, W), 177, np.uint8), np.full((H, W), 177, np.uint8)
    good_h = dict(e=eng._h, l=h["dl"].ctypes.data, r=h["dr"].ctypes.data, b=h["base"].ctypes.data, H=H, W=W, invalid=-16, T=24, rad=r,
                  V=2304, cl=hcl.ctypes.data, cr=hcr.ctypes.data)
    good_1 = dict(good_h, l=dl[0].data_ptr(), r=dr[0].data_ptr(), b=b[0].data_ptr(), cl=cl[0].data_ptr(), cr=cr[0].data_ptr())
    good_n = dict(good_h, N=N, l=arr(dl), r=arr(dr), b=arr(b), cl=arr(cl), cr=arr(cr))
    bad = [dict(e=None), dict(l=None), dict(r=None), dict(cl=None, cr=None), dict(H=0), dict(W=-1), dict(H=-3), dict(invalid=32768),
           dict(invalid=-32769), dict(T=-1), dict(T=32768), dict(rad=-1), dict(rad=17), dict(V=0), dict(V=-7), dict(V=(1 << 30) + 1)]
    alias = lambda g: [dict(cl=g["l"]), dict(cl=g["r"]), dict(cr=g["b"]), dict(cr=g["l"]), dict(cr=g["cl"])]
    one = lambda fn, a: fn(a["e"], a["l"], a["r"], a["b"], a["H"], a["W"], a["invalid"], a["T"], a["rad"], a["V"], a["cl"], a["cr"])
    many = lambda fn, a: fn(a["e"], a["N"], a["l"], a["r"], a["b"], a["H"], a["W"], a["invalid"], a["T"], a["rad"], a["V"], a["cl"], a["cr"])
    holes = [dict(N=0), dict(N=-2), dict(l=arr(dl, 1)), dict(r=arr(dr, 0)), dict(b=arr(b, 2)), dict(cl=arr(cl, 2)), dict(cr=arr(cr, 1)),
             dict(cl=mixed(cl, 1, dl[2])), dict(cr=mixed(cr, 0, b[1])), dict(cr=mixed(cr, 2, cl[0])), dict(cl=mixed(cl, 0, cl[1]))]
    checks = [(one, L.sgm_lrc_confidence, good_h, alias(good_h)), (one, L.sgm_lrc_confidence_device, good_1, alias(good_1)),
              (many, L.sgm_lrc_confidence_batch_device, good_n, holes)]
    for call, fn, good, more in checks:
        for bd in bad + more:
            assert call(fn, dict(good, **bd)) == -1, bd                  # SGM_ERR_INVALID_ARG
            assert b"sgm_lrc_confidence" in L.sgm_last_error(), bd
            # ... and a correct call follows each
            assert call(fn, good) == 0, (_lib.last_error(), bd)
            eng.synchronize()
            if fn is L.sgm_lrc_confidence:
                _same(hcl, wants[0][0]), _same(hcr, wants[0][1])
                hcl[:], hcr[:] = 177, 177
            else:
                n = N if call is many else 1
                gl, gr = cl.cpu().numpy(), cr.cpu().numpy()
                for k in range(n):
                    _same(gl[k], wants[k][0], bd), _same(gr[k], wants[k][1], bd)
                cl.fill_(177), cr.fill_(177)
                torch.cuda.synchronize()
    # nothing is enqueued by a refused call: the markers stand
    for call, fn, good, more in checks:
        for bd in bad + more:
            assert call(fn, dict(good, **bd)) == -1
    eng.synchronize()
    assert (hcl == 177).all() and (hcr == 177).all() and (cl.cpu().numpy() == 177).all() and (cr.cpu().numpy() == 177).all()


# ---- 4. history -------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_the_engine_did_before():
    e = Engine(P16)
    big, small = 7, 4                      # 97 x 260, then 64 x 64
    def run(i, entry):
        H, W, r, T, V, invalid, levels = LR.SHAPE_CASES[i]
        s = LR.case_input(i)
        if entry == "host":
            got = e.lrc_confidence_host(s["dl"], s["dr"], s["base"], invalid, T, r, V, True, True)
        else:
            got = [g[0] for g in _device(e, [s], True, invalid, T, r, V)]
        _same(got[0], LR.case_want(i)[0], (i, entry, "left")), _same(got[1], LR.case_want(i)[1], (i, entry, "right"))
    run(small, "host")
    run(big, "device")
    run(small, "device")                   # a smaller shape in the larger planes
    run(big, "host")
    e.trim()                               # gives the factor planes back; they return on the next call
    run(small, "device")
    try:
        for byte in (0xA5, 0x7F):
            e.set_option(_lib.SGM_OPT_POISON, byte)      # fills every buffer the engine owns and arms the same for new ones
            run(small, "host")
            e.set_option(_lib.SGM_OPT_POISON, byte)
            run(big, "device")
            run(small, "device")
    finally:
        e.set_option(_lib.SGM_OPT_POISON, -1)


def test_the_profile_record_names_the_two_stages():
    e = Engine(P16)
    pairs = [_pair(65, 129, 300 + k, -160, 6, 24, 2304) for k in range(5)]
    ins, wants = [p[0] for p in pairs], [p[1] for p in pairs]
    try:
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        e.set_option(_lib.SGM_OPT_GROUP_MAX, 2)          # 5 pairs: three chunks in one record
        cl, cr = _device(e, ins, True, -160, 24, 6, 2304)
        st = {n: (ms, launches) for n, ms, launches in e.stage_times()}
        assert set(st) == {"lrc_factor", "lrc_match", "_wall"}, st
        assert (st["lrc_factor"][1], st["lrc_match"][1]) == (3, 3), st
        assert all(ms >= 0 for ms, _ in st.values())
        for k in range(5):
            _same(cl[k], wants[k][0]), _same(cr[k], wants[k][1])
        got = e.lrc_confidence_host(ins[0]["dl"], ins[0]["dr"], ins[0]["base"], -160, 24, 6, 2304, True, True)   # a single call: one launch each
        st = {n: launches for n, ms, launches in e.stage_times()}
        assert st == {"lrc_factor": 1, "lrc_match": 1, "_wall": 0}, st
        _same(got[0], wants[0][0])
        # the filter's record is its own, as before
        f32 = cv.wls_weights(1.5)
        e.wls_filter_host(ins[0]["dl"], np.zeros((65, 129), np.uint8), got[0], -160, 8000.0, f32)
        assert {n for n, _, _ in e.stage_times()} == {"wls_init", "wls_rows", "wls_cols", "wls_final", "_wall"}
    finally:
        e.set_option(_lib.SGM_OPT_PROFILE, 0)
        e.set_option(_lib.SGM_OPT_GROUP_MAX, 0)


# ---- 5. the Python surface: lrcConfidence, the filter with a right map ----------------------------------------------------------------
def test_lrc_confidence_with_numpy_and_with_tensors():
    import torch
    s, (wl, wr) = _pair(65, 129, 11, -16, 5, 24, 2304)
    _same(cv.lrcConfidence(s["dl"], s["dr"], s["base"]), wl)                 # the defaults: -16, 24, 5, 2304
    got = cv.lrcConfidence(s["dl"], s["dr"], s["base"], return_right=True)
    _same(got[0], wl), _same(got[1], wr)
    t = lambda a: torch.from_numpy(a.copy()).cuda()
    got = cv.lrcConfidence(t(s["dl"]), t(s["dr"]), t(s["base"]), return_right=True)
    assert got[0].is_cuda and got[0].dtype == torch.uint8
    _same(got[0].cpu().numpy(), wl), _same(got[1].cpu().numpy(), wr)
    s2, (wl2, _) = _pair(33, 97, 12, -160, 2, 8, 500, with_base=False)
    _same(cv.lrcConfidence(s2["dl"], s2["dr"], invalid=-160, thresh=8, radius=2, var_max=500), wl2)
    _same(cv.lrcConfidence(t(s2["dl"]), t(s2["dr"]), invalid=-160, thresh=8, radius=2, var_max=500).cpu().numpy(), wl2)


def test_the_filter_with_a_right_map_is_the_filter_with_the_reference_confidence():
    import torch
    H, W = 65, 129
    s, _ = _pair(H, W, 21, -16, 5, 24, 2304)
    rng = np.random.default_rng(5)
    guide = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    t = lambda a: torch.from_numpy(a.copy()).cuda()
    for base in (s["base"], None):
        f = cv.createDisparityWLSFilter()                                   # no matcher: radius 5, invalid -16
        f.setLRCthresh(20)
        f.setDiscontinuityVariance(1500)
        ref = LR.lrc_confidence(s["dl"], s["dr"], base, -16, 20, 5, 1500)[0]
        want = f.filter(s["dl"], guide, confidence=ref)
        assert (want != s["dl"]).any()
        with pytest.raises(cv.error, match="getConfidenceMap"):
            f.getConfidenceMap()                                            # a call without a right map keeps none
        got = f.filter(s["dl"], guide, confidence=base, disparity_map_right=s["dr"])
        assert np.array_equal(got, want)
        _same(f.getConfidenceMap(), ref)
        got = f.filter(t(s["dl"]), t(guide), None if base is None else t(base), disparity_map_right=t(s["dr"]))
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
        assert f.getConfidenceMap().is_cuda
        _same(f.getConfidenceMap().cpu().numpy(), ref)
    # cv2's call shape: wls.filter(disp_left, left, None, disp_right) -- here the fourth POSITIONAL argument stays `invalid`
    m = cv.StereoSGBM_create(minDisparity=-9, numDisparities=16, blockSize=7)
    f = cv.createDisparityWLSFilter(m)                                      # radius 4, invalid -160
    s2, _ = _pair(33, 97, 22, -160, 4, 24, 2304)
    ref = LR.lrc_confidence(s2["dl"], s2["dr"], None, -160, 24, 4, 2304)[0]
    assert np.array_equal(f.filter(s2["dl"], guide[:33, :97, 0].copy(), None, disparity_map_right=s2["dr"]),
                          f.filter(s2["dl"], guide[:33, :97, 0].copy(), ref))
    _same(f.getConfidenceMap(), ref)


def test_filter_batch_with_right_maps():
    import torch
    N, H, W = 3, 33, 97
    pairs = [_pair(H, W, 31 + k, -16, 5, 24, 2304) for k in range(N)]
    ins, wants = [p[0] for p in pairs], [p[1] for p in pairs]
    rng = np.random.default_rng(6)
    guides = rng.integers(0, 256, (N, H, W)).astype(np.uint8)
    st = lambda key: np.stack([s[key] for s in ins])
    refs = np.stack([w[0] for w in wants])
    f = cv.createDisparityWLSFilter()
    want = f.filterBatch(st("dl"), guides, refs)
    got = f.filterBatch(st("dl"), guides, st("base"), disparity_maps_right=st("dr"))
    assert np.array_equal(got, want)
    assert f.getConfidenceMap().shape == (N, H, W)
    _same(f.getConfidenceMap(), refs)
    t = lambda a: torch.from_numpy(a.copy()).cuda()
    got = f.filterBatch(t(st("dl")), t(guides), [t(s["base"]) for s in ins], disparity_maps_right=[t(s["dr"]) for s in ins])
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert f.getConfidenceMap().is_cuda and tuple(f.getConfidenceMap().shape) == (N, H, W)
    _same(f.getConfidenceMap().cpu().numpy(), refs)
    for i in range(N):                                                      # every map equals filter() on it alone
        assert np.array_equal(f.filter(ins[i]["dl"], guides[i], ins[i]["base"], disparity_map_right=ins[i]["dr"]), want[i])
    # without base
    refs0 = np.stack([LR.lrc_confidence(s["dl"], s["dr"], None, -16, 24, 5, 2304)[0] for s in ins])
    assert np.array_equal(f.filterBatch(st("dl"), guides, disparity_maps_right=st("dr")), f.filterBatch(st("dl"), guides, refs0))
    _same(f.getConfidenceMap(), refs0)


# ---- 6. computeFiltered -----------------------------------------------------------------------------------------------------------
def _chain(m, left, right, source, lambda_=8000.0, sigmaColor=1.5):
    """computeFiltered(confidence=source) assembled by hand: computeLeftRight, computeWithConfidence, lrcConfidence, filter"""
    dl, dr = m.computeLeftRight(left, right)
    dl2, margin = m.computeWithConfidence(left, right)
    same = (lambda a, b: bool((a == b).all())) if cv._is_torch(dl) else np.array_equal
    assert same(dl, dl2)
    f = cv.createDisparityWLSFilter(m)
    f.setLambda(lambda_)
    f.setSigmaColor(sigmaColor)
    conf = cv.lrcConfidence(dl, dr, margin if source == "both" else None, invalid=f.defaultInvalid(), thresh=24,
                            radius=f.getDepthDiscontinuityRadius(), var_max=2304)
    return f.filter(dl, left, conf), conf


def test_compute_filtered_with_the_lr_confidence_equals_the_chain_by_hand():
    import torch
    gray = [synth.make_pair(48, 320, 64, 7 + i)[:2] for i in range(3)]
    colour = [BC.colour_pair(48, 320, 64, seed=22 + i) for i in range(3)]
    for pairs, p in ((gray, U.params(64, 5, 0, 1)), (colour, U.params(64, 3, 0, 1, penalty="plain"))):
        m = cv.StereoSGBM_create(**p)
        a, b = pairs[0]
        plain = m.computeFiltered(a, b)
        assert np.array_equal(m.computeFiltered(a, b, confidence="margin"), plain)
        wants = {}
        for source in ("lrc", "both"):
            want, conf = _chain(m, a, b, source)
            # the confidence does something on this pair: zeros, full confidence and values in between all occur (the scene is
            # piecewise constant, so there are few distinct ones)
            assert (conf != 0).mean() > 0.25 and len(np.unique(conf)) >= 3 and conf.min() == 0 and conf.max() == 100
            got = m.computeFiltered(a, b, confidence=source)
            assert got.dtype == np.int16 and np.array_equal(got, want), (source, int((got != want).sum()))
            assert not np.array_equal(got, plain)
            wants[source] = want
        assert not np.array_equal(wants["lrc"], wants["both"])
        got = m.computeFiltered(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), confidence="both")
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), wants["both"])
        assert np.array_equal(m.computeFiltered(a, b), plain)                    # the cached engine goes back as it was
        assert np.array_equal(m.compute(a, b), m.computeWithConfidence(a, b)[0])
        # the batch form: result i equals the single call, numpy and tensors
        lefts, rights = np.stack([x for x, _ in pairs]), np.stack([y for _, y in pairs])
        assert np.array_equal(m.computeFilteredBatch(lefts, rights, confidence="margin"), m.computeFilteredBatch(lefts, rights))
        for source in ("lrc", "both"):
            single = [m.computeFiltered(x, y, confidence=source) for x, y in pairs]
            assert np.array_equal(single[0], wants[source]) and not np.array_equal(single[0], single[1])
            got = m.computeFilteredBatch(lefts, rights, confidence=source)
            assert isinstance(got, np.ndarray) and got.shape == lefts.shape[:3]
            for i in range(3):
                assert np.array_equal(got[i], single[i]), (source, i, int((got[i] != single[i]).sum()))
            t = m.computeFilteredBatch(torch.from_numpy(lefts).cuda(), [torch.from_numpy(y).cuda() for _, y in pairs], confidence=source)
            assert t.is_cuda and np.array_equal(t.cpu().numpy(), got)


def test_one_1080p_pair_through_both():
    """the real map sizes once: 1080 x 1920, D = 128, on the device from end to end"""
    import torch
    a, b = synth.make_pair(1080, 1920, 128, seed=5)[:2]
    m = cv.StereoSGBM_create(**U.params(128, 5, 0, 1))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    want, conf = _chain(m, ta, tb, "both")
    got = m.computeFiltered(ta, tb, confidence="both")
    assert torch.equal(got, want), int((got != want).sum())
    assert float((conf != 0).float().mean()) > 0.25


# ---- 7. guarded buffers -----------------------------------------------------------------------------------------------------------
def test_the_shape_list_with_every_buffer_guarded():
    """(the same shapes ran in the plain mode above: test_shapes_through_every_entry)"""
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lrc_guard_child.py")], capture_output=True, text=True, env=env,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"LRC_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) == NCASE, tail
