"""The batch form of the edge-aware disparity filter on the device (needs an MI355X): sgm_wls_filter_batch,
sgm_wls_filter_batch_device, DisparityWLSFilter.filterBatch, StereoSGBM.computeFilteredBatch.

Yardstick: tests/wls_ref.py in float32 on every map alone -- the definition of include/sgm_hip_wls.h -- bit for bit: the int16
map directly, the float map through its bit pattern (the comparison of tests/test_gpu_wls.py: _same).  Every map of a batch has
a seed of its own, so a mixed-up map index shows.  Only the full-size case is held against single device calls instead (the
numpy reference is too slow there)."""
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

# (N, H, W, cn, conf): one map; degenerate lines; one full tile; the row kernel's tile edges with a tail workgroup and a tail
# tile; three row workgroups; more maps than a small chunk; two column waves; a partial fifth tile with colour.  invalid
# alternates between -16 and -160; (lambda, sigma) are those of WR.SHAPE_CASES, case by case.
SHAPES = [(1, 65, 129, 1, True), (2, 1, 7, 3, False), (3, 7, 1, 1, True), (2, 1, 1, 1, True), (5, 64, 64, 3, True),
          (4, 65, 129, 1, True), (3, 130, 67, 3, False), (17, 33, 97, 1, True), (2, 200, 33, 1, True), (3, 97, 260, 3, True)]
CASES = [s + WR.SHAPE_CASES[i][4:6] + ((-16, -160)[i % 2],) for i, s in enumerate(SHAPES)]


@functools.lru_cache(maxsize=None)
def _weights(sigma):
    return WR.weights(sigma)


@functools.lru_cache(maxsize=None)
def _map(H, W, cn, with_conf, lam, sigma, invalid, seed, holes=0.3):
    """(input, reference) of ONE map, computed once and shared; nobody writes to either"""
    s = WR.random_input(H, W, cn, seed, invalid, holes, with_conf)
    want = WR.wls_filter(s["disp"], s["guide"], s["conf"], invalid, lam, _weights(sigma))
    for a in list(s.values()) + list(want.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return s, want


def _batch(N, H, W, cn, with_conf, lam, sigma, invalid, seed0=1000):
    """N maps with the seeds seed0 .. seed0 + N - 1: (list of inputs, list of references)"""
    maps = [_map(H, W, cn, with_conf, lam, sigma, invalid, seed0 + i) for i in range(N)]
    return [m[0] for m in maps], [m[1] for m in maps]


def _stack(ins, key):
    return None if ins[0][key] is None else np.stack([s[key] for s in ins])


def _same(out, outf, want, what=""):
    assert out.dtype == np.int16 and np.array_equal(out, want["out"]), (what, int((out != want["out"]).sum()))
    if outf is not None:
        assert outf.dtype == np.float32
        nbad = int((outf.view(np.uint32) != want["out_f32"].view(np.uint32)).sum())
        assert nbad == 0, (what, nbad)


def _same_all(outs, outfs, wants, what=""):
    assert len(outs) == len(wants)
    for i, w in enumerate(wants):
        _same(outs[i], None if outfs is None else outfs[i], w, (what, "map", i))


def _host(eng, ins, invalid, lam, sigma):
    return eng.wls_filter_batch_host(_stack(ins, "disp"), _stack(ins, "guide"), _stack(ins, "conf"), invalid, lam, _weights(sigma),
                                     return_float=True)


def _device(eng, ins, invalid, lam, sigma, with_float=True):
    """every map in a tensor of its own (so neighbours in the batch are not neighbours in memory); the outputs pre-filled"""
    import torch
    dev = torch.device("cuda", eng.device)
    H, W = ins[0]["disp"].shape
    cn = 1 if ins[0]["guide"].ndim == 2 else 3
    t = lambda key: None if ins[0][key] is None else [torch.from_numpy(s[key].copy()).to(dev) for s in ins]
    d, g, c = t("disp"), t("guide"), t("conf")
    out = [torch.full((H, W), 77, dtype=torch.int16, device=dev) for _ in ins]
    outf = [torch.full((H, W), 7.0, dtype=torch.float32, device=dev) for _ in ins] if with_float else None
    ptrs = lambda ts: None if ts is None else [x.data_ptr() for x in ts]
    torch.cuda.synchronize()
    eng.wls_filter_batch_device(ptrs(d), ptrs(g), cn, ptrs(c), H, W, invalid, lam, _weights(sigma), ptrs(out), ptrs(outf))
    eng.synchronize()
    for i, s in enumerate(ins):      # inputs untouched
        assert np.array_equal(d[i].cpu().numpy(), s["disp"]) and np.array_equal(g[i].cpu().numpy(), s["guide"])
        assert c is None or np.array_equal(c[i].cpu().numpy(), s["conf"])
    return [x.cpu().numpy() for x in out], None if outf is None else [x.cpu().numpy() for x in outf]


@pytest.fixture(scope="module")
def eng():
    return Engine(P16)


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,cn,with_conf,lam,sigma,invalid", CASES)
def test_shapes_through_both_entries(eng, N, H, W, cn, with_conf, lam, sigma, invalid):
    ins, wants = _batch(N, H, W, cn, with_conf, lam, sigma, invalid)
    out, outf = _host(eng, ins, invalid, lam, sigma)
    assert out.shape == (N, H, W) and outf.shape == (N, H, W)
    _same_all(out, outf, wants, ("host", N, H, W, cn))
    _same_all(*_device(eng, ins, invalid, lam, sigma), wants, ("device", N, H, W, cn))
    if H * W > 100:
        assert all(0 < w["valid"].sum() and (w["out"] != s["disp"]).any() for s, w in zip(ins, wants))     # the case does something
        assert N == 1 or not np.array_equal(wants[0]["out"], wants[1]["out"])                              # ... per map


def test_an_all_invalid_and_an_all_valid_map_between_ordinary_ones(eng):
    case = (65, 129, 1, True, 8000.0, 1.5, -16)
    maps = [_map(*case, seed=20), _map(*case, seed=21, holes=2.0), _map(*case, seed=22), _map(*case, seed=23, holes=-1.0),
            _map(*case, seed=24)]
    ins, wants = [m[0] for m in maps], [m[1] for m in maps]
    assert (ins[1]["disp"] == -16).all() and (ins[3]["disp"] != -16).all()
    for out, outf in (_host(eng, ins, -16, 8000.0, 1.5), _device(eng, ins, -16, 8000.0, 1.5)):
        _same_all(out, outf, wants)      # (the ordinary neighbours 0, 2, 4 among them)
        assert (out[1] == -16).all() and (outf[1].view(np.uint32) == 0).all()


# ---- 2. chunks --------------------------------------------------------------------------------------------------------------------
def test_chunks_give_the_same_results():
    """N = 5 in chunks of 2 + 2 + 1 and of 1 x 5 (SGM_OPT_GROUP_MAX) against one chunk, through both entries"""
    e = Engine(P16)
    N, H, W, cn, with_conf, lam, sigma, invalid = CASES[4][:1] + (65, 129, 3, True, 8000.0, 1.5, -160)
    ins, wants = _batch(N, H, W, cn, with_conf, lam, sigma, invalid, seed0=40)
    try:
        for gm in (0, 2, 1, 0):
            e.set_option(_lib.SGM_OPT_GROUP_MAX, gm)
            _same_all(*_host(e, ins, invalid, lam, sigma), wants, ("host, group_max", gm))
            _same_all(*_device(e, ins, invalid, lam, sigma), wants, ("device, group_max", gm))
    finally:
        e.set_option(_lib.SGM_OPT_GROUP_MAX, 0)


# ---- 3. the batch is N single calls -------------------------------------------------------------------------------------------------
def test_the_batch_equals_single_device_calls(eng):
    import torch
    dev = torch.device("cuda", eng.device)
    N, H, W, lam, sigma, invalid = 4, 65, 129, 8000.0, 1.5, -16
    lut = _weights(sigma)
    for cn in (1, 3):
        ins, wants = _batch(N, H, W, cn, True, lam, sigma, invalid, seed0=60)
        up = lambda a: torch.from_numpy(a.copy()).to(dev)
        d, g, c = [up(s["disp"]) for s in ins], [up(s["guide"]) for s in ins], [up(s["conf"]) for s in ins]
        single, singlef = [], []
        for i in range(N):
            o, of = torch.full((H, W), 77, dtype=torch.int16, device=dev), torch.full((H, W), 7.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            eng.wls_filter_device(d[i].data_ptr(), g[i].data_ptr(), cn, c[i].data_ptr(), H, W, invalid, lam, lut, o.data_ptr(), of.data_ptr())
            eng.synchronize()
            single.append(o.cpu().numpy())
            singlef.append(of.cpu().numpy())
        _same_all(single, singlef, wants, "single calls")
        ptrs = lambda ts: [x.data_ptr() for x in ts]
        # outputs pre-filled with a marker; inputs untouched
        out = [torch.full((H, W), 77, dtype=torch.int16, device=dev) for _ in range(N)]
        outf = [torch.full((H, W), 7.0, dtype=torch.float32, device=dev) for _ in range(N)]
        torch.cuda.synchronize()
        eng.wls_filter_batch_device(ptrs(d), ptrs(g), cn, ptrs(c), H, W, invalid, lam, lut, ptrs(out), ptrs(outf))
        eng.synchronize()
        for i in range(N):
            assert np.array_equal(out[i].cpu().numpy(), single[i]), (cn, i)
            assert np.array_equal(outf[i].cpu().numpy().view(np.uint32), singlef[i].view(np.uint32)), (cn, i)
            assert np.array_equal(d[i].cpu().numpy(), ins[i]["disp"]) and np.array_equal(g[i].cpu().numpy(), ins[i]["guide"])
            assert np.array_equal(c[i].cpu().numpy(), ins[i]["conf"])
        # no float map, and in place: out[i] is disp[i]
        d2 = [x.clone() for x in d]
        torch.cuda.synchronize()
        eng.wls_filter_batch_device(ptrs(d2), ptrs(g), cn, ptrs(c), H, W, invalid, lam, lut, ptrs(d2), None)
        eng.synchronize()
        for i in range(N):
            assert np.array_equal(d2[i].cpu().numpy(), single[i]), ("in place", cn, i)
        # no confidence array, one guide shared by all maps
        out = [torch.full((H, W), 77, dtype=torch.int16, device=dev) for _ in range(N)]
        torch.cuda.synchronize()
        eng.wls_filter_batch_device(ptrs(d), [g[1].data_ptr()] * N, cn, None, H, W, invalid, lam, lut, ptrs(out), None)
        eng.synchronize()
        for i in range(N):
            o = torch.full((H, W), 77, dtype=torch.int16, device=dev)
            torch.cuda.synchronize()
            eng.wls_filter_device(d[i].data_ptr(), g[1].data_ptr(), cn, None, H, W, invalid, lam, lut, o.data_ptr(), None)
            eng.synchronize()
            assert np.array_equal(out[i].cpu().numpy(), o.cpu().numpy()), ("shared guide, no confidence", cn, i)
            _same(o.cpu().numpy(), None, WR.wls_filter(ins[i]["disp"], ins[1]["guide"], None, invalid, lam, lut))
    # the host entry in place, no float map, no confidence
    ins, _ = _batch(3, 130, 67, 3, False, 100.0, 10.0, -16)
    buf, guides = _stack(ins, "disp").copy(), _stack(ins, "guide")
    lut = _weights(10.0)
    rc = _lib.load().sgm_wls_filter_batch(eng._h, 3, buf.ctypes.data, guides.ctypes.data, 3, None, 130, 67, -16, C.c_double(100.0),
                                          lut.ctypes.data, buf.ctypes.data, None)
    assert rc == 0, _lib.last_error()
    _same_all(buf, None, _batch(3, 130, 67, 3, False, 100.0, 10.0, -16)[1], "host in place")


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(eng):
    import torch
    L = _lib.load()
    N, H, W = 3, 65, 129
    ins, wants = _batch(N, H, W, 1, True, 8000.0, 1.5, -16, seed0=80)
    lut = _weights(1.5)
    dev = torch.device("cuda", eng.device)
    hd, hg, hc = _stack(ins, "disp"), _stack(ins, "guide"), _stack(ins, "conf")
    hout = np.full((N, H, W), 77, np.int16)
    dd, dg, dc = (torch.from_numpy(a.copy()).to(dev) for a in (hd, hg, hc))
    dout = torch.full((N, H, W), 77, dtype=torch.int16, device=dev)
    doutf = torch.full((N, H, W), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    arr = lambda t, hole=None: (C.c_void_p * N)(*[None if i == hole else t[i].data_ptr() for i in range(N)])
    good = dict(e=eng._h, N=N, disp=hd.ctypes.data, guide=hg.ctypes.data, cn=1, conf=hc.ctypes.data, H=H, W=W, invalid=-16, lam=8000.0,
                lut=lut.ctypes.data, out=hout.ctypes.data, outf=None)
    good_d = dict(good, disp=arr(dd), guide=arr(dg), conf=arr(dc), out=arr(dout), outf=arr(doutf))
    bad = [dict(N=0), dict(N=-2), dict(disp=None), dict(guide=None), dict(out=None), dict(lut=None), dict(e=None), dict(H=0), dict(W=-1),
           dict(cn=2), dict(cn=0), dict(lam=-1.0), dict(lam=1e7 + 1), dict(lam=float("nan")), dict(invalid=32768), dict(invalid=-32769)]
    holes = [dict(disp=arr(dd, 1)), dict(guide=arr(dg, 0)), dict(conf=arr(dc, 2)), dict(out=arr(dout, 2)), dict(outf=arr(doutf, 1))]
    call = lambda fn, a: fn(a["e"], a["N"], a["disp"], a["guide"], a["cn"], a["conf"], a["H"], a["W"], a["invalid"], C.c_double(a["lam"]),
                            a["lut"], a["out"], a["outf"])
    for fn, base, more in ((L.sgm_wls_filter_batch, good, []), (L.sgm_wls_filter_batch_device, good_d, holes)):
        for b in bad + more:
            assert call(fn, dict(base, **b)) == -1, b                 # SGM_ERR_INVALID_ARG
            assert b"sgm_wls_filter" in L.sgm_last_error()
    eng.synchronize()
    assert (hout == 77).all() and (dout.cpu().numpy() == 77).all() and (doutf.cpu().numpy() == 7.0).all()     # nothing was enqueued
    assert call(L.sgm_wls_filter_batch, good) == 0, _lib.last_error()
    _same_all(hout, None, wants)
    assert call(L.sgm_wls_filter_batch_device, good_d) == 0, _lib.last_error()
    eng.synchronize()
    _same_all(dout.cpu().numpy(), doutf.cpu().numpy(), wants)


# ---- 5. history -------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_the_engine_did_before():
    e = Engine(P16)
    small, big = CASES[5], CASES[9]           # 4 x 65 x 129 gray, 3 x 97 x 260 colour
    run = lambda case, entry: entry(e, _batch(*case)[0], case[7], case[5], case[6])
    first = run(small, _host)
    _same_all(*first, _batch(*small)[1], "fresh engine")
    _same_all(*run(big, _device), _batch(*big)[1], "the larger shape")
    _same_all(*run(small, _device), _batch(*small)[1], "after a larger shape")
    s1, w1 = _map(*WR.SHAPE_CASES[8], seed=0)
    _same(*e.wls_filter_host(s1["disp"], s1["guide"], s1["conf"], -160, 8000.0, _weights(0.5), return_float=True), w1, "a single map between")
    _same_all(*run(small, _host), _batch(*small)[1], "after a single-map call")
    e.trim()                                   # gives the planes back; they return on the next call
    _same_all(*run(small, _device), _batch(*small)[1], "after sgm_trim")
    try:
        for byte in (0xA5, 0x7F):
            e.set_option(_lib.SGM_OPT_POISON, byte)      # fills every buffer the engine owns and arms the same for new ones
            got = run(small, _host)
            _same_all(*got, _batch(*small)[1], ("poisoned", byte))
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1].view(np.uint32), first[1].view(np.uint32))
            e.set_option(_lib.SGM_OPT_POISON, byte)
            _same_all(*run(big, _device), _batch(*big)[1], ("poisoned, device entry", byte))
    finally:
        e.set_option(_lib.SGM_OPT_POISON, -1)


def test_the_profile_record_names_the_four_stages():
    e = Engine(P16)
    ins, wants = _batch(*CASES[5])
    try:
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        e.set_option(_lib.SGM_OPT_GROUP_MAX, 3)          # 4 maps: two chunks in one record
        _same_all(*_device(e, ins, CASES[5][7], CASES[5][5], CASES[5][6]), wants)
        st = {n: (ms, launches) for n, ms, launches in e.stage_times()}
        assert set(st) == {"wls_init", "wls_rows", "wls_cols", "wls_final", "_wall"}, st
        assert (st["wls_init"][1], st["wls_rows"][1], st["wls_cols"][1], st["wls_final"][1]) == (2, 6, 6, 2), st
        assert all(ms >= 0 for ms, _ in st.values())
    finally:
        e.set_option(_lib.SGM_OPT_PROFILE, 0)
        e.set_option(_lib.SGM_OPT_GROUP_MAX, 0)


# ---- 6. the Python surface ---------------------------------------------------------------------------------------------------------
def test_filter_batch_with_tensors_and_with_numpy():
    import torch
    N, H, W, cn, with_conf, lam, sigma, invalid = CASES[9]
    ins, wants = _batch(N, H, W, cn, with_conf, lam, sigma, invalid)
    f = cv.createDisparityWLSFilter()
    f.setLambda(lam)
    f.setSigmaColor(sigma)
    t = lambda a: torch.from_numpy(a.copy()).cuda()
    # a stacked tensor
    out, outf = f.filterBatch(t(_stack(ins, "disp")), t(_stack(ins, "guide")), t(_stack(ins, "conf")), invalid=invalid, return_float=True)
    assert out.is_cuda and outf.is_cuda and out.dtype == torch.int16 and outf.dtype == torch.float32 and tuple(out.shape) == (N, H, W)
    _same_all(out.cpu().numpy(), outf.cpu().numpy(), wants, "stacked tensors")
    # a sequence of tensors
    out = f.filterBatch([t(s["disp"]) for s in ins], [t(s["guide"]) for s in ins], [t(s["conf"]) for s in ins], invalid=invalid)
    assert out.is_cuda and tuple(out.shape) == (N, H, W)
    _same_all(out.cpu().numpy(), None, wants, "a sequence of tensors")
    # numpy: a stack, and a sequence
    got, gotf = f.filterBatch(_stack(ins, "disp"), _stack(ins, "guide"), _stack(ins, "conf"), invalid=invalid, return_float=True)
    assert isinstance(got, np.ndarray) and got.shape == (N, H, W)
    _same_all(got, gotf, wants, "numpy stack")
    got = f.filterBatch([s["disp"] for s in ins], [s["guide"] for s in ins], [s["conf"] for s in ins], invalid=invalid)
    _same_all(got, None, wants, "numpy sequence")
    # every map equals filter() on it alone
    for i, s in enumerate(ins):
        assert np.array_equal(f.filter(s["disp"], s["guide"], s["conf"], invalid=invalid), got[i])
    with pytest.raises(cv.error, match="CUDA"):
        f.filterBatch(t(_stack(ins, "disp")), _stack(ins, "guide"))
    # no confidence; the default invalid value comes from the matcher
    N2, _, _, _, _, lam2, sigma2, inv2 = CASES[7]
    assert inv2 == -160
    ins2, wants2 = _batch(*CASES[7])
    f2 = cv.createDisparityWLSFilter(cv.StereoSGBM_create(minDisparity=-9, numDisparities=16))
    f2.setLambda(lam2)
    f2.setSigmaColor(sigma2)
    _same_all(f2.filterBatch(_stack(ins2, "disp"), _stack(ins2, "guide"), _stack(ins2, "conf")), None, wants2, "matcher's invalid")


def test_compute_filtered_batch_equals_compute_filtered_pair_by_pair():
    import torch
    gray = [synth.make_pair(48, 320, 64, 7 + i)[:2] for i in range(3)]
    colour = [BC.colour_pair(48, 320, 64, seed=22 + i) for i in range(3)]
    for pairs, p in ((gray, U.params(64, 5, 0, 1)), (colour, U.params(64, 3, 0, 1, penalty="plain"))):
        m = cv.StereoSGBM_create(**p)
        lefts, rights = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
        want = [m.computeFiltered(a, b) for a, b in pairs]
        assert not np.array_equal(want[0], want[1])
        got = m.computeFilteredBatch(lefts, rights)
        assert isinstance(got, np.ndarray) and got.dtype == np.int16 and got.shape == lefts.shape[:3]
        for i in range(3):
            assert np.array_equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
        t = m.computeFilteredBatch(torch.from_numpy(lefts).cuda(), [torch.from_numpy(b).cuda() for _, b in pairs])
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), got)
        other = m.computeFilteredBatch([a for a, _ in pairs], [b for _, b in pairs], lambda_=500.0, sigmaColor=3.0)
        for i, (a, b) in enumerate(pairs):
            assert np.array_equal(other[i], m.computeFiltered(a, b, lambda_=500.0, sigmaColor=3.0)), i
        assert np.array_equal(m.computeFiltered(*pairs[0]), want[0])       # the cached engine goes back as it was


# ---- 7. full size -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _full_size_inputs():
    """three maps 2160 x 4096 with guide and confidence (a piecewise map with noise and 20 % holes over a guide that follows it)"""
    H, W = 2160, 4096
    res = []
    for seed in range(3):
        rng = np.random.default_rng(900 + seed)
        layer = np.add.outer(np.arange(H) // (97 + seed), np.arange(W) // (131 - seed)) % 3
        disp = (np.array([200, 420, 600])[layer] + rng.integers(-24, 25, (H, W))).astype(np.int16)
        disp[rng.random((H, W), np.float32) < 0.2] = -16
        gray = (np.array([60, 120, 180])[layer] + rng.integers(-2, 3, (H, W))).astype(np.uint8)
        res.append((disp, gray, rng.integers(0, 101, (H, W)).astype(np.uint8)))
    return res


@pytest.mark.parametrize("W", [3840, 4096])
def test_full_size_n64_against_single_device_calls(W):
    """4K, N = 64, one chunk: two inputs alternate and a third is the last map, every map with output buffers of its own; maps
    0, 1, 62 and 63 against sgm_wls_filter_device on them alone.  The planes of a chunk lie at 64-bit offsets: at 3840 x 2160 the
    64 float planes end at byte 2 123 366 400, just BELOW 2^31, so the same is run at 4096 x 2160 (DCI 4K), where the planes of
    maps 61 .. 63 begin past 2^31 (map 63: byte 2 229 534 720) -- a 32-bit byte offset would show in maps 62 and 63 there."""
    import torch
    H, N = 2160, 64
    e = Engine(P16)
    dev = torch.device("cuda", e.device)
    lut = _weights(1.5)
    src = [tuple(torch.from_numpy(np.ascontiguousarray(a[:, :W])).to(dev) for a in trio) for trio in _full_size_inputs()]
    which = [i % 2 for i in range(N - 1)] + [2]
    out = [torch.full((H, W), 77, dtype=torch.int16, device=dev) for _ in range(N)]
    outf = [torch.full((H, W), 7.0, dtype=torch.float32, device=dev) for _ in range(N)]
    torch.cuda.synchronize()
    e.wls_filter_batch_device([src[k][0].data_ptr() for k in which], [src[k][1].data_ptr() for k in which], 1,
                              [src[k][2].data_ptr() for k in which], H, W, -16, 8000.0, lut, [x.data_ptr() for x in out],
                              [x.data_ptr() for x in outf])
    e.synchronize()
    one, onef = torch.empty((H, W), dtype=torch.int16, device=dev), torch.empty((H, W), dtype=torch.float32, device=dev)
    for i in (0, 1, 62, 63):
        d, g, c = src[which[i]]
        e.wls_filter_device(d.data_ptr(), g.data_ptr(), 1, c.data_ptr(), H, W, -16, 8000.0, lut, one.data_ptr(), onef.data_ptr())
        e.synchronize()
        assert torch.equal(out[i], one), (i, int((out[i] != one).sum()))
        assert torch.equal(outf[i].view(torch.int32), onef.view(torch.int32)), i
        assert int((one != -16).sum()) > 0.9 * H * W and not torch.equal(one, d)       # the filter did something
    assert not torch.equal(out[0], out[1]) and not torch.equal(out[62], out[63]) and torch.equal(out[0], out[62])
    e.trim()


# ---- 8. guarded buffers -----------------------------------------------------------------------------------------------------------
def test_batches_with_every_buffer_guarded():
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wls_batch_guard_child.py")], capture_output=True, text=True,
                       env=env, timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"WLS_BATCH_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) == 6, tail
