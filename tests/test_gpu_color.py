"""Colour (8-bit, 3-channel) pairs through the engine (needs an MI355X): SGM_OPT_CHANNELS = 3, k_features<3> + k_hsum<., ., 3>
into the int16 vertical box sum.  Checked against an implementation-independent known answer, against the C oracle through
two exact relations (the block cost is the sum of the three channel images' block costs; (I, I, I) with tripled penalties
is the gray map of I) and end to end against the colour brute force of tests/bruteforce_color.py."""
import ctypes as C

import numpy as np
import pytest

import bruteforce_color as BC
import parity_util as U
from oracle import oracle as O
from oracle import volume_oracle as V
from stereo_reconstruction_cv_amd import _lib, pipeline, synth
from stereo_reconstruction_cv_amd import stereo as cv
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu


def _engine(p, schedule=1, sweep_rows=0, chain_wgs=0):
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, schedule)
    eng.set_option(_lib.SGM_OPT_SWEEP_ROWS, sweep_rows)
    if chain_wgs:
        eng.set_option(_lib.SGM_OPT_CHAIN_WGS, chain_wgs)
    return eng


def _oracle_channel_C(L, R, p):
    """the oracle's C taps of the three channel images (int32 sum) and whether every channel stayed in the regime (only
    the C tap is asked for: a 4K D=256 volume is 4 GB)"""
    H, W = L.shape[:2]
    pr = O.make_params(**p)
    _, W1 = O.geometry(pr, W)
    total = np.zeros((H, W1, p["numDisparities"]), np.int32)
    Cc = np.empty(total.shape, np.int16)
    disp = np.empty((H, W), np.int16)
    ok = True
    for c in range(3):
        l, r = np.ascontiguousarray(L[..., c]), np.ascontiguousarray(R[..., c])
        t = O.Taps()
        t.C = Cc.ctypes.data
        assert O.lib().oracle_sgbm_compute(C.byref(pr), l.ctypes.data, r.ctypes.data, H, W, W, disp.ctypes.data, C.byref(t)) == 0
        total += Cc
        ok = ok and bool(t.headroom_ok)
    return total, ok


def _equal(a, b, rows=64):
    """a == b element for element, row block by row block (no full-size temporaries for 4K volumes)"""
    return a.shape == b.shape and all(np.array_equal(a[y:y + rows].astype(np.int32), b[y:y + rows].astype(np.int32))
                                      for y in range(0, a.shape[0], rows))


# ---- 1. option semantics ---------------------------------------------------------------------------------------------
def test_channels_option_values_and_stride():
    p = U.params(16, 3)
    eng = Engine(p)
    for v in (1, 3, 1):
        eng.set_option(_lib.SGM_OPT_CHANNELS, v)
    for v in (0, 2, 4, -1):
        with pytest.raises(cv.error, match="SGM_OPT_CHANNELS"):
            eng.set_option(_lib.SGM_OPT_CHANNELS, v)
    # stride < 3 W is refused by every image entry point that takes one
    H, W = 8, 40
    eng.set_option(_lib.SGM_OPT_CHANNELS, 3)
    img = np.zeros((H, W, 3), np.uint8)
    out = np.empty((H, W), np.int16)
    L = _lib.load()
    assert L.sgm_compute(eng._h, img.ctypes.data, img.ctypes.data, H, W, 3 * W - 1, out.ctypes.data) == -1
    assert "stride" in _lib.last_error()
    import torch
    t = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    d = torch.empty((H, W), dtype=torch.int16, device="cuda")
    assert L.sgm_compute_device(eng._h, t.data_ptr(), t.data_ptr(), H, W, 3 * W - 1, d.data_ptr()) == -1
    assert L.sgm_pipeline_device(eng._h, t.data_ptr(), t.data_ptr(), H, W, 2 * W, None, d.data_ptr(), None, None) == -1
    arr = (C.c_void_p * 1)(t.data_ptr())
    darr = (C.c_void_p * 1)(d.data_ptr())
    assert L.sgm_pipeline_batch_device(eng._h, 1, arr, arr, H, W, 3 * W - 1, None, darr, None, None) == -1
    assert L.sgm_compute(eng._h, img.ctypes.data, img.ctypes.data, H, W, 3 * W, out.ctypes.data) == 0


def test_gray_after_colour_on_the_same_engine():
    H, W, D = 40, 200, 64
    p = U.params(D, 5)
    L3, R3 = BC.colour_pair(H, W, D, seed=3)
    I, J, _ = synth.make_pair(H, W, D, seed=4)
    eng = Engine(p)
    eng.compute_host(L3, R3)
    got = eng.compute_host(I, J)
    assert np.array_equal(got, Engine(p).compute_host(I, J))
    assert np.array_equal(got, O.sgbm_compute(I, J, **p))


# ---- 2. known answer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs,ok", [(7, True), (11, False)])
def test_constant_pair_known_answer(bs, ok):
    """0 against 255 in every channel: the gradient planes are flat (ftzero), the raw planes differ by 255 -> 63 per
    channel, so the interior block cost is bs^2 * 3 * 63 (9261 at bs = 7).  With the notebook's penalties the regime holds at
    bs = 7 and is left at bs = 11 (121 * 189 + 11616 > 32767)."""
    H, W, D = 30, 160, 16
    r = bs // 2
    p = U.params(D, bs)
    L3, R3 = np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8)
    eng = Engine(p)
    eng.compute_host(L3, R3)
    Cg = eng.tap(_lib.SGM_TAP_COST, H, W)
    minX1, W1 = eng.geometry(W)
    # columns whose window (and the half-pixel intervals around it) stays clear of the border columns 0 and W-1
    xi = np.arange(W1)
    x = xi + minX1
    clear = (x - (D - 1) - r - 1 >= 1) & (x + r + 1 <= W - 2)
    assert clear.sum() > 20
    assert (Cg[:, clear] == bs * bs * 3 * 63).all()
    hr = eng.headroom()
    assert hr["ok"] is ok, hr
    assert hr["max_cost_plus_p2"] >= bs * bs * 189 + p["P2"]


# ---- 3. linearity of the block cost --------------------------------------------------------------------------------------
LIN = [  # H, W, D, minD, bs, mode, cap, P1, P2
    (720, 1280, 64, 0, 5, 0, 63, 200, 800),
    (1080, 1920, 128, 0, 5, 1, 63, 200, 800),
    (48, 300, 16, 0, 5, 0, 63, 40, 160),
    (40, 320, 32, -5, 3, 1, 15, 18, 72),
    (40, 300, 48, 0, 1, 0, 63, 8, 32),
    (36, 700, 512, -3, 7, 0, 111, 98, 392),
    (40, 500, 192, 0, 5, 1, 63, 50, 200),                 # NP = 2 (D 129 .. 256)
    (36, 560, 256, -4, 3, 0, 63, 18, 72),
    (2160, 3840, 256, 0, 7, 0, 63, 8 * 3 * 49, 32 * 3 * 49),   # the bench's shape, notebook penalties, both modes
    (2160, 3840, 256, 0, 7, 1, 63, 8 * 3 * 49, 32 * 3 * 49),
    (40, 360, 96, 0, 15, 1, 15, 30, 135),
    (40, 400, 128, 0, 17, 0, 15, 34, 153),
    (24, 90, 16, 0, 19, 1, 15, 38, 171),
    # k_hsum<NP, RS_T, 3> instantiations at W1 just above one 128-column chunk (the second chunk is short and mostly takes
    # the generic step)
    (30, 420, 256, 0, 13, 1, 15, 26, 117),                # NP = 2, RS_T = 16
    (30, 400, 192, 0, 19, 0, 15, 38, 171),                # NP = 2 partial, RS_T = 0
    (30, 660, 512, 0, 3, 1, 63, 18, 72),                  # NP = 4, RS_T = 4
    (30, 640, 480, -2, 13, 0, 15, 26, 117),               # NP = 4 partial, RS_T = 16
    (30, 660, 512, 0, 17, 1, 15, 34, 153),                # NP = 4, RS_T = 0
]


@pytest.mark.parametrize("H,W,D,minD,bs,mode,cap,P1,P2", LIN)
def test_colour_cost_is_the_sum_of_the_channel_costs(H, W, D, minD, bs, mode, cap, P1, P2):
    p = dict(U.NB, minDisparity=minD, numDisparities=D, blockSize=bs, P1=P1, P2=P2, mode=mode, preFilterCap=cap)
    L3, R3 = BC.colour_pair(H, W, D, seed=H + W + D + bs, minD=minD)
    want, ok = _oracle_channel_C(L3, R3, p)
    eng = Engine(p)
    eng.compute_host(L3, R3)
    got = eng.tap(_lib.SGM_TAP_COST, H, W)
    hr = eng.headroom()
    assert ok and hr["ok"], hr
    assert int(want.max()) + p["P2"] <= hr["max_cost_plus_p2"] <= 32767
    assert _equal(got, want)


# ---- 4. end to end against the colour brute force ------------------------------------------------------------------------
E2E = [  # H, W, D, minD, bs, mode, schedule, sweep_rows, chain_wgs
    (12, 64, 16, 0, 3, 0, 1, 0, 0),
    (12, 72, 32, -2, 5, 1, 1, 0, 0),
    (13, 110, 64, 0, 3, 0, 1, 3, 0),
    (14, 120, 64, 1, 5, 1, 1, 4, 0),
    (12, 90, 48, 0, 1, 1, 0, 0, 0),
    (12, 100, 64, 0, 5, 0, 2, 3, 2),
    (15, 120, 64, -3, 3, 1, 2, 4, 2),
    (12, 100, 48, 0, 3, 1, 2, 2, 3),
    (12, 300, 192, 0, 3, 1, 1, 3, 0),                     # NP = 2
    (12, 330, 256, -2, 3, 0, 2, 3, 2),
    (14, 420, 256, 0, 5, 1, 0, 0, 0),
]


@pytest.mark.parametrize("H,W,D,minD,bs,mode,schedule,rows,wgs", E2E)
def test_end_to_end_against_the_colour_brute_force(H, W, D, minD, bs, mode, schedule, rows, wgs):
    p = U.params(D, bs, minD, mode, penalty="plain", speckleWindowSize=12, speckleRange=2)
    L3, R3 = BC.colour_pair(H, W, D, seed=11 * H + D + bs + schedule, minD=minD)
    want = BC.sgbm_c3(L3, R3, **p)
    eng = _engine(p, schedule, rows, wgs)
    got = eng.compute_host(L3, R3)
    assert eng.headroom()["ok"]
    assert np.array_equal(eng.tap(_lib.SGM_TAP_COST, H, W), want["C"])
    assert np.array_equal(eng.tap(_lib.SGM_TAP_DISP_RAW, H, W), want["disp_raw"])
    assert np.array_equal(eng.tap(_lib.SGM_TAP_DISP_MEDIAN, H, W), want["disp_median"])
    assert np.array_equal(got, want["disp"])
    assert (got > (minD - 1) * 16).mean() > 0.2   # not a degenerate case


# ---- 5. equal channels, full size ------------------------------------------------------------------------------------------
def _wta_reads_unsaturated(S, uniq, k=3, rows=64):
    for y in range(0, S.shape[0], rows):   # (row blocks: a 4K D=256 volume is 4 GB)
        Sw = S[y:y + rows].astype(np.int32)
        m = Sw.min(axis=2, keepdims=True)
        read = Sw * (100 - uniq) < m * 100 + 1               # the uniqueness band (includes the best d)
        best = Sw.argmin(axis=2)[..., None]
        for o in (-1, 1):
            np.put_along_axis(read, np.clip(best + o, 0, S.shape[2] - 1), True, axis=2)
        if int(Sw[read].max()) * k >= 32767:
            return False
    return True


@pytest.mark.parametrize("H,W,D,bs,mode,k1,k2", [(2160, 3840, 256, 5, 1, 1, 4), (2160, 3840, 128, 5, 0, 2, 8),
                                                 (1080, 1920, 128, 5, 0, 2, 8), (1080, 1920, 128, 5, 1, 2, 8),
                                                 (720, 1280, 64, 5, 1, 2, 8)])
def test_equal_channels_full_size(H, W, D, bs, mode, k1, k2):
    """(I, I, I) with penalties (3 P1, 3 P2) is the gray map of I with (P1, P2) = (k1 bs^2, k2 bs^2), bit for bit on the
    whole frame, given that no value the winner-take-all reads saturates once tripled (asserted from the oracle's S tap;
    the notebook's penalties tripled, or bs = 7 at 4K D = 256 with eight paths, would break it on this input)."""
    I, J, _ = synth.make_pair(H, W, D, seed=900 + D + mode)
    pg = U.params(D, bs, 0, mode, P1=k1 * bs * bs, P2=k2 * bs * bs)
    gray, t = O.sgbm_compute(I, J, taps=True, **pg)
    assert t["headroom_ok"] and 3 * t["max_delta"] <= 32767
    assert _wta_reads_unsaturated(t["S"], pg["uniquenessRatio"])
    del t["S"]
    eng = Engine(dict(pg, P1=3 * pg["P1"], P2=3 * pg["P2"]))
    got = eng.compute_host(np.repeat(I[..., None], 3, axis=2), np.repeat(J[..., None], 3, axis=2))
    assert eng.headroom()["ok"]
    Cg = eng.tap(_lib.SGM_TAP_COST, H, W)
    assert all(np.array_equal(Cg[y:y + 64].astype(np.int32), 3 * t["C"][y:y + 64].astype(np.int32)) for y in range(0, H, 64))
    del Cg
    assert np.array_equal(eng.tap(_lib.SGM_TAP_DISP_RAW, H, W), t["disp_raw"])
    assert np.array_equal(got, gray), int((got != gray).sum())


@pytest.mark.parametrize("schedule", [1, 2])
def test_full_hd_colour_pair_against_the_volume_oracle(schedule):
    """1920 x 1080, D = 128, bs = 5, MODE_HH on three DIFFERENT channels: every map and the headroom record against the
    volume oracle (oracle/sgbm_volume_oracle.c, pinned by tests/test_volume_oracle.py) -- the relations above reach full
    size only through gray images in disguise."""
    H, W, D = 1080, 1920, 128
    p = U.params(D, 5, 0, 1, penalty="plain", speckleWindowSize=60, speckleRange=2)
    L3, R3 = BC.colour_pair(H, W, D, seed=1080)
    want, t = _full_hd_colour_oracle()
    eng = _engine(p, schedule)
    got = eng.compute_host(L3, R3)
    eng.check()
    assert eng.headroom() == dict(ok=True, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"])
    assert np.array_equal(eng.tap(_lib.SGM_TAP_DISP_RAW, H, W), t["disp_raw"])
    assert np.array_equal(eng.tap(_lib.SGM_TAP_DISP_MEDIAN, H, W), t["disp_median"])
    assert np.array_equal(got, want), int((got != want).sum())


_full_hd = []


def _full_hd_colour_oracle():
    if not _full_hd:
        H, W, D = 1080, 1920, 128
        p = U.params(D, 5, 0, 1, penalty="plain", speckleWindowSize=60, speckleRange=2)
        want, t = V.sgbm_compute(*BC.colour_pair(H, W, D, seed=1080), taps="light", **p)
        assert t["headroom_ok"] and (want >= 0).mean() > 0.5, (t["max_cost_plus_p2"], t["max_delta"], (want >= 0).mean())
        _full_hd.append((want, t))
    return _full_hd[0]


# ---- 6. batches ------------------------------------------------------------------------------------------------------------
BH, BW, BD = 24, 180, 64


def _batch_pairs(n):
    return [BC.colour_pair(BH, BW, BD, seed=700 + i) for i in range(n)]


@pytest.mark.parametrize("schedule,gmax,N", [(1, 0, 4), (2, 0, 3), (2, 2, 5)])
def test_host_batch_of_colour_pairs(schedule, gmax, N):
    p = U.params(BD, 5, 0, 1, penalty="plain", speckleWindowSize=12, speckleRange=2)
    pairs = _batch_pairs(N)
    single = Engine(p)
    want = [single.compute_host(a, b) for a, b in pairs]
    hmax = 0
    for i, (a, b) in enumerate(pairs):
        single.compute_host(a, b)
        hmax = max(hmax, single.headroom()["max_cost_plus_p2"])
    bf = BC.sgbm_c3(*pairs[0], **p)["disp"]
    assert np.array_equal(want[0], bf)
    eng = _engine(p, schedule, 4)
    if gmax:
        eng.set_option(_lib.SGM_OPT_GROUP_MAX, gmax)
    Q = synth.default_Q(BW)
    disps, xyz = eng.compute_batch_host(np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]), Q)
    for i in range(N):
        assert np.array_equal(disps[i], want[i]), (i, int((disps[i] != want[i]).sum()))
    hr = eng.headroom()
    assert hr["ok"]
    if schedule == 2:   # throughput mode: the record covers every pair of the call (schedule 1 keeps its peers' records apart)
        assert hr["max_cost_plus_p2"] == hmax
    # a gray batch on the same engine afterwards is gray again
    gp = [synth.make_pair(BH, BW, BD, 40 + i)[:2] for i in range(N)]
    gd = eng.compute_batch_host(np.stack([a for a, _ in gp]), np.stack([b for _, b in gp]))
    for i, (a, b) in enumerate(gp):
        assert np.array_equal(gd[i], O.sgbm_compute(a, b, **p)), i


@pytest.mark.parametrize("gmax", [0, 2])
def test_resident_batch_of_colour_pairs(gmax):
    import torch
    p = U.params(BD, 5, 0, 0, penalty="plain", speckleWindowSize=12, speckleRange=2)
    N = 5
    pairs = _batch_pairs(N)
    single = Engine(p)
    want = [single.compute_host(a, b) for a, b in pairs]
    dev = torch.device("cuda", 0)
    dl = [torch.from_numpy(a).to(dev) for a, _ in pairs]
    dr = [torch.from_numpy(b).to(dev) for _, b in pairs]
    dd = [torch.full((BH, BW), -7, dtype=torch.int16, device=dev) for _ in range(N)]
    torch.cuda.synchronize()
    eng = _engine(p, 2, 4)
    if gmax:
        eng.set_option(_lib.SGM_OPT_GROUP_MAX, gmax)
    # a gray batch of the same shape first: the group engines then grow for the colour plan (prepare_group)
    g0 = [synth.make_pair(BH, BW, BD, 80 + i)[:2] for i in range(N)]
    gl0 = [torch.from_numpy(a).to(dev) for a, _ in g0]
    gr0 = [torch.from_numpy(b).to(dev) for _, b in g0]
    torch.cuda.synchronize()
    eng.pipeline_batch_device([t.data_ptr() for t in gl0], [t.data_ptr() for t in gr0], BH, BW, BW, None,
                              [t.data_ptr() for t in dd])
    eng.synchronize()
    for i, (a, b) in enumerate(g0):
        assert np.array_equal(dd[i].cpu().numpy(), O.sgbm_compute(a, b, **p)), i
    eng.pipeline_batch_device([t.data_ptr() for t in dl], [t.data_ptr() for t in dr], BH, BW, 3 * BW, None,
                              [t.data_ptr() for t in dd], cn=3)
    eng.synchronize()
    for i in range(N):
        assert np.array_equal(dd[i].cpu().numpy(), want[i]), i
    assert eng.headroom()["ok"]
    # gray pairs through the same engine afterwards
    gp = [synth.make_pair(BH, BW, BD, 60 + i)[:2] for i in range(N)]
    gl = [torch.from_numpy(a).to(dev) for a, _ in gp]
    gr = [torch.from_numpy(b).to(dev) for _, b in gp]
    torch.cuda.synchronize()
    eng.pipeline_batch_device([t.data_ptr() for t in gl], [t.data_ptr() for t in gr], BH, BW, BW, None,
                              [t.data_ptr() for t in dd])
    eng.synchronize()
    for i, (a, b) in enumerate(gp):
        assert np.array_equal(dd[i].cpu().numpy(), O.sgbm_compute(a, b, **p)), i


# ---- 7. Python surface -------------------------------------------------------------------------------------------------------
def test_stereo_sgbm_compute_layouts_and_torch():
    import torch
    H, W, D = 32, 160, 32
    p = U.params(D, 5)
    L3, R3 = BC.colour_pair(H, W + 20, D, seed=21)
    m = cv.StereoSGBM_create(**p)
    a, b = np.ascontiguousarray(L3[:, :W]), np.ascontiguousarray(R3[:, :W])
    want = BC.sgbm_c3(a, b, **p)["disp"]
    assert np.array_equal(m.compute(a, b), want)
    # a cropped view (pixel stride 3, padded rows) passes as it is
    assert np.array_equal(m.compute(L3[:, :W], R3[:, :W]), want)
    # the BGR channels of a BGRA array (pixel stride 4) are copied
    bgra_l = np.concatenate([a, np.full((H, W, 1), 9, np.uint8)], axis=2)
    bgra_r = np.concatenate([b, np.full((H, W, 1), 200, np.uint8)], axis=2)
    assert np.array_equal(m.compute(bgra_l[..., :3], bgra_r[..., :3]), want)
    # channel order does not matter (BGR and RGB give the same map)
    assert np.array_equal(m.compute(a[..., ::-1], b[..., ::-1]), want)
    # HIP tensors
    out = m.compute(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert out.is_cuda and out.dtype == torch.int16 and np.array_equal(out.cpu().numpy(), want)
    # gray after colour through the cached engine
    I, J, _ = synth.make_pair(H, W, D, seed=22)
    assert np.array_equal(m.compute(I, J), O.sgbm_compute(I, J, **p))


def test_notebook_function_on_a_colour_pair():
    H, W, D = 40, 200, 32
    L3, R3 = BC.colour_pair(H, W, D, seed=31)
    f = pipeline.compute_disparity_map(L3, R3, D, 0)
    p = dict(minDisparity=0, numDisparities=D, blockSize=11, P1=8 * 3 * 121, P2=32 * 3 * 121, disp12MaxDiff=1,
             preFilterCap=63, uniquenessRatio=10, speckleWindowSize=100, speckleRange=32)
    d16 = cv.StereoSGBM_create(**p).compute(L3, R3).astype(np.float32) / 16
    assert f.dtype == np.float32 and np.array_equal(f, d16 * (d16 > 0))
    xyz = pipeline.reconstruct_3D(f, synth.default_Q(W))
    assert xyz is not None and xyz.shape == (H, W, 3)


def test_cv2_style_errors():
    import torch
    m = cv.StereoSGBM_create(numDisparities=16)
    z = lambda *s: np.zeros(s, np.uint8)
    for bad in ((z(8, 40, 2), z(8, 40, 2)), (z(8, 40, 4), z(8, 40, 4))):
        with pytest.raises(cv.error, match="channels"):
            m.compute(*bad)
    with pytest.raises(cv.error, match="Assertion failed"):
        m.compute(z(8, 40, 3), z(8, 40))                     # colour left, gray right
    with pytest.raises(cv.error, match="Assertion failed"):
        m.compute(z(8, 40, 3), z(8, 41, 3))
    with pytest.raises(cv.error, match="Assertion failed"):
        m.compute(z(8, 40, 3), np.zeros((8, 40, 3), np.uint16))
    t = torch.zeros((8, 40, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(cv.error, match="channels"):
        m.compute(t, t)
