"""numDisparities 528 ... 1024 on the GPU (needs an MI355X): 16 disparities per lane (NP = 8) through k_hsum (gray and colour),
the element-wise vertical sum and one k_path launch per direction, bit for bit against the oracles.

Yardsticks: gray pairs in modes 0 and 1 -- the frozen oracle (oracle/sgbm_oracle.c); MODE_HH4 and colour pairs -- the
volume oracle (oracle/sgbm_volume_oracle.c, pinned by tests/test_volume_oracle.py).  Every comparison is exact, on every tap
(C, S, disp_raw, disp_median, disp) and on the headroom record.  No case is skipped: the oracle keeps every row inside the
int16 regime (the last column of ROWS is its max C + P2), and the tests assert that.
(upstream counterpart of what the kernels compute: /root/reference/main.ipynb:668 -> SURVEY.md A.2-A.8)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bruteforce_color as BC
import parity_util as U
from oracle import oracle as O
from oracle import volume_oracle as V
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd import stereo as cv
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# H, W, D, bs, minD, mode, extra arguments, the oracle's max C + P2
ROWS = [
    (31, 1400, 528, 3, 0, 0, {}, 2390),
    (37, 1500, 1024, 5, 0, 1, {}, 5920),
    (29, 1700, 768, 7, 3, 1, {}, 10153),
    (33, 1419, 1008, 5, -7, 0, {}, 5936),
    (23, 1250, 640, 9, 0, 1, {}, 15825),
    (27, 1300, 896, 13, 0, 0, {}, 28655),
    (21, 1300, 544, 15, 0, 1, dict(penalty="plain"), 24748),
    (19, 1500, 1024, 3, 0, 0, dict(uniquenessRatio=100), 2375),                      # POSW = false
    (25, 1500, 1024, 5, 0, 1, dict(uniquenessRatio=0, disp12MaxDiff=-1), 5755),
    (24, 1600, 1024, 21, 0, 0, dict(P1=50, P2=400), 29822),
    (24, 1600, 784, 31, 0, 1, dict(P1=20, P2=90, preFilterCap=15), 30763),
    (40, 1600, 1024, 11, 0, 1, {}, 22792),
    (25, 1030, 1024, 5, 0, 1, {}, 5097),                                             # W1 = 6
    (12, 900, 1024, 5, 0, 0, {}, 0),                                                 # W1 <= 0: all invalid
]
row_id = lambda r: f"{r[0]}x{r[1]} D{r[2]} bs{r[3]} minD{r[4]} mode{r[5]}" + "".join(f" {k}={v}" for k, v in r[6].items())


def row_case(r):
    H, W, D, bs, minD, mode, kw, _ = r
    l, rt, _ = synth.make_pair(H, W, D, 9000 + D + bs)
    return l, rt, U.params(D, bs, minD, mode, **kw)


_oracle = {}


def oracle_of(r):
    """the frozen oracle's taps for a row (cached: the schedules of a row share them)"""
    if r[:6] + (tuple(sorted(r[6].items())),) not in _oracle:
        l, rt, p = row_case(r)
        d, t = O.sgbm_compute(l, rt, taps=True, **p)
        t["disp"] = d
        t["headroom"] = dict(ok=bool(t["headroom_ok"]), max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"])
        _oracle[r[:6] + (tuple(sorted(r[6].items())),)] = t
    return _oracle[r[:6] + (tuple(sorted(r[6].items())),)]


def check_row(r, schedule, **opts):
    l, rt, p = row_case(r)
    t = oracle_of(r)
    assert t["headroom_ok"] and t["max_cost_plus_p2"] == r[7], (t["max_cost_plus_p2"], t["max_delta"])
    h = U.run_hip_with_taps(l, rt, p, schedule, **opts)
    keys = [k for k in ("C", "S", "disp_raw", "disp_median", "disp") if k in t]
    assert [k for k in keys if k not in h] == []
    bad = [U.describe_mismatch(k, h[k], t[k]) for k in keys if not np.array_equal(h[k], t[k])]
    if h["headroom"] != t["headroom"]:
        bad.append(U.describe_mismatch("headroom", h["headroom"], t["headroom"]))
    assert not bad, f"{row_id(r)} schedule {schedule} {opts}: " + "\n".join(bad)
    return h, t


@pytest.mark.parametrize("schedule", [0, 1, 2])
@pytest.mark.parametrize("r", ROWS, ids=[row_id(r) for r in ROWS])
def test_every_stage_against_the_frozen_oracle(r, schedule):
    h, t = check_row(r, schedule)
    W1 = r[1] + min(r[4], 0) - max(r[4] + r[2], 0)
    if W1 > 0:
        assert h["C"].shape == (r[0], W1, r[2]) and h["S"].shape == h["C"].shape
    else:
        assert "C" not in h and (h["disp"] == (r[4] - 1) * 16).all()


@pytest.mark.parametrize("opts", [dict(sweep_rows=5, prepass_rows=64, chain_wgs=3), dict(debug=2), dict(debug=4), dict(debug=16),
                                  dict(debug=256), dict(debug=2048)], ids=str)
@pytest.mark.parametrize("schedule", [1, 2])
def test_schedule_options_are_accepted_and_change_nothing(schedule, opts):
    check_row(ROWS[2], schedule, **opts)


def test_profile_names_the_per_direction_route():
    for r, want in ((ROWS[1], ["path_S", "path_SE", "path_SW", "path_N", "path_NE", "path_NW", "path_E", "path_W_wta"]),
                    (ROWS[0], ["path_S", "path_SE", "path_SW", "path_E", "path_W_wta"])):
        l, rt, p = row_case(r)
        for schedule in (1, 2):
            eng = Engine(p)
            eng.set_option(_lib.SGM_OPT_SCHEDULE, schedule)
            eng.set_option(_lib.SGM_OPT_PROFILE, 1)
            got = eng.compute_host(l, rt)
            assert np.array_equal(got, oracle_of(r)["disp"])
            names = [n for n, _, _ in eng.stage_times()]
            assert names[:3] == ["features", "cost_hsum", "cost_vsum"], names
            assert [n for n in names if n.startswith("path")] == want, names
            assert not [n for n in names if n.startswith(("sweep", "chain", "prepass", "cost_pix", "cost_box")) or n == "wta"], names


# ---- full size ------------------------------------------------------------------------------------------------------------
def test_full_hd_1024_disparities_mode_hh():
    H, W, D, bs = 1080, 1920, 1024, 7
    l, rt, _ = synth.make_pair(H, W, D, 9000 + D + bs)
    p = U.params(D, bs, 0, 1)
    want, t = O.sgbm_compute(l, rt, taps="light", **p)
    valid = (want >= 0).mean()
    print(f"1080p D=1024 mode 1: oracle max C + P2 {t['max_cost_plus_p2']}, max delta {t['max_delta']}, valid {valid:.3f}")
    assert t["headroom_ok"] and valid > 0.3
    eng = Engine(p)
    got = eng.compute_host(l, rt)
    assert eng.headroom() == dict(ok=True, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"])
    assert np.array_equal(eng.tap(_lib.SGM_TAP_DISP_RAW, H, W), t["disp_raw"])
    assert np.array_equal(eng.tap(_lib.SGM_TAP_DISP_MEDIAN, H, W), t["disp_median"])
    assert np.array_equal(got, want), int((got != want).sum())


def test_4k_1024_disparities_mode_sgbm():
    """Volumes of 12.5 GB each (hsum, C, S): every address product beyond 32 bits."""
    H, W, D, bs = 2160, 3840, 1024, 7
    l, rt, _ = synth.make_pair(H, W, D, 9000 + D + bs)
    p = U.params(D, bs, 0, 0)
    want, t = O.sgbm_compute(l, rt, taps="light", **p)
    valid = (want >= 0).mean()
    print(f"4K D=1024 mode 0: oracle max C + P2 {t['max_cost_plus_p2']}, max delta {t['max_delta']}, valid {valid:.3f}")
    assert t["headroom_ok"] and valid > 0.6
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, 2)
    got = eng.compute_host(l, rt)
    assert eng.headroom() == dict(ok=True, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"])
    assert np.array_equal(got, want), int((got != want).sum())


# ---- MODE_HH4 and colour pairs against the volume oracle ------------------------------------------------------------------
def _volume_case(l, rt, p, schedule, label):
    want, t = V.sgbm_compute(l, rt, taps=True, **p)
    assert t["headroom_ok"], (label, t["max_cost_plus_p2"], t["max_delta"])
    t["disp"] = want
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_KEEP_AGGR, 1)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, schedule)
    H, W = l.shape[:2]
    h = dict(disp=eng.compute_host(l, rt), C=eng.tap(_lib.SGM_TAP_COST, H, W), S=eng.tap(_lib.SGM_TAP_AGGR, H, W),
             disp_raw=eng.tap(_lib.SGM_TAP_DISP_RAW, H, W), disp_median=eng.tap(_lib.SGM_TAP_DISP_MEDIAN, H, W))
    bad = [U.describe_mismatch(k, h[k], t[k]) for k in ("C", "S", "disp_raw", "disp_median", "disp") if not np.array_equal(h[k], t[k])]
    hr = dict(ok=True, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"])
    if eng.headroom() != hr:
        bad.append(f"headroom record: hip {eng.headroom()} != {hr}")
    assert not bad, f"{label} schedule {schedule}: " + "\n".join(bad)
    return h


@pytest.mark.parametrize("schedule", [0, 1, 2])
@pytest.mark.parametrize("H,W,D,bs", [(25, 1300, 640, 5), (33, 1500, 1024, 3)])
def test_mode_hh4_against_the_volume_oracle(H, W, D, bs, schedule):
    l, rt, _ = synth.make_pair(H, W, D, seed=11)
    h = _volume_case(l, rt, U.params(D, bs, 0, 3), schedule, f"HH4 {H}x{W} D{D}")
    assert (h["disp"] >= 0).any()


@pytest.mark.parametrize("mode", [0, 1, 3])
@pytest.mark.parametrize("H,W,D,bs,schedule", [(21, 1200, 528, 5, 1), (23, 1500, 1024, 3, 2)])
def test_colour_pairs_against_the_volume_oracle(H, W, D, bs, schedule, mode):
    L3, R3 = BC.colour_pair(H, W, D, seed=H + W + D + bs)
    p = U.params(D, bs, 0, mode, penalty="plain", speckleWindowSize=12, speckleRange=2)
    _volume_case(L3, R3, p, schedule, f"colour {H}x{W} D{D} mode {mode}")


# ---- entry points ---------------------------------------------------------------------------------------------------------
EH, EW, ED = 26, 1500, 1024


def _entry_pairs(n):
    return [synth.make_pair(EH, EW, ED, 9500 + i)[:2] for i in range(n)]


def test_stereo_sgbm_compute_on_numpy_and_on_hip_tensors():
    import torch
    p = U.params(ED, 5, 0, 1)
    l, rt = _entry_pairs(1)[0]
    want = O.sgbm_compute(l, rt, **p)
    st = cv.StereoSGBM_create(**p)
    got = st.compute(l, rt)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    dev = torch.device("cuda", 0)
    gt = st.compute(torch.from_numpy(l).to(dev), torch.from_numpy(rt).to(dev))
    assert isinstance(gt, torch.Tensor) and gt.is_cuda and np.array_equal(gt.cpu().numpy(), want)
    with pytest.raises(cv.error, match="1024"):
        cv.StereoSGBM_create(**dict(p, numDisparities=1040)).compute(l, rt)


def test_pipeline_device_float_map_and_xyz():
    import torch
    p = U.params(ED, 5, 0, 0)
    l, rt = _entry_pairs(1)[0]
    want = O.sgbm_compute(l, rt, **p)
    Q = synth.default_Q(EW)
    dev = torch.device("cuda", 0)
    dl, dr = torch.from_numpy(l).to(dev), torch.from_numpy(rt).to(dev)
    dd = torch.full((EH, EW), -9, dtype=torch.int16, device=dev)
    df = torch.zeros((EH, EW), dtype=torch.float32, device=dev)
    dx = torch.zeros((EH, EW, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    eng = Engine(p)
    eng.pipeline_device(dl.data_ptr(), dr.data_ptr(), EH, EW, EW, Q, dd.data_ptr(), df.data_ptr(), dx.data_ptr())
    eng.synchronize()
    assert np.array_equal(dd.cpu().numpy(), want)
    f = O.disp_to_float(want)
    assert np.array_equal(df.cpu().numpy(), f)
    ref = O.reproject(f, Q)
    xyz = dx.cpu().numpy()
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(xyz), fin) and np.allclose(xyz[fin], ref[fin], rtol=1e-4, atol=0.0)


@pytest.mark.parametrize("schedule", [1, 2])
def test_batch_entries_equal_single_computes(schedule):
    import torch
    p = U.params(ED, 5, 0, 1)
    pairs = _entry_pairs(4)
    single = Engine(p)
    want, hmax, dmax = [], 0, 0
    for a, b in pairs:
        want.append(single.compute_host(a, b))
        hr = single.headroom()
        assert hr["ok"]
        hmax, dmax = max(hmax, hr["max_cost_plus_p2"]), max(dmax, hr["max_delta"])
    assert np.array_equal(want[0], O.sgbm_compute(*pairs[0], **p))
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, schedule)
    # four pairs from host memory
    disps = eng.compute_batch_host(np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]))
    for i in range(4):
        assert np.array_equal(disps[i], want[i]), (i, int((disps[i] != want[i]).sum()))
    assert eng.headroom() == dict(ok=True, max_cost_plus_p2=hmax, max_delta=dmax)
    # three resident pairs
    dev = torch.device("cuda", 0)
    dl = [torch.from_numpy(a).to(dev) for a, _ in pairs[:3]]
    dr = [torch.from_numpy(b).to(dev) for _, b in pairs[:3]]
    dd = [torch.full((EH, EW), -7, dtype=torch.int16, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    eng.pipeline_batch_device([t.data_ptr() for t in dl], [t.data_ptr() for t in dr], EH, EW, EW, None, [t.data_ptr() for t in dd])
    eng.synchronize()
    eng.check()
    for i in range(3):
        assert np.array_equal(dd[i].cpu().numpy(), want[i]), i
    h3, d3 = 0, 0
    for a, b in pairs[:3]:
        single.compute_host(a, b)
        h3, d3 = max(h3, single.headroom()["max_cost_plus_p2"]), max(d3, single.headroom()["max_delta"])
    assert eng.headroom() == dict(ok=True, max_cost_plus_p2=h3, max_delta=d3)


# ---- history ----------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_ran_before():
    """An engine's arguments are fixed when it is created (sgm_create), so "D = 256, then 1024, then 256" is one MATCHER
    whose numDisparities is set back and forth -- its engines take turns on the device -- and, on the D = 1024 engine itself,
    a walk over shapes: large, small, large again, then the same with every device buffer filled with 0xA5."""
    A, B = (30, 1500), (17, 1200)
    case = {}
    for D, (H, W) in ((256, A), (1024, A), (1024, B)):
        l, rt, _ = synth.make_pair(H, W, D, 9600 + D + H)
        p = U.params(D, 5, 0, 1)
        d, t = O.sgbm_compute(l, rt, taps=True, **p)
        assert t["headroom_ok"]
        case[D, H] = (l, rt, p, d, t)
    narrow, wide = Engine(case[256, 30][2]), Engine(case[1024, 30][2])
    narrow.set_option(_lib.SGM_OPT_SCHEDULE, 2)      # chained
    wide.set_option(_lib.SGM_OPT_SCHEDULE, 2)
    wide.set_option(_lib.SGM_OPT_KEEP_AGGR, 1)

    def run(eng, D, H, W):
        l, rt, p, want, t = case[D, H]
        assert np.array_equal(eng.compute_host(l, rt), want), (D, H)
        eng.check()
        assert eng.headroom() == dict(ok=True, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"]), (D, H)
        if eng is wide:
            assert np.array_equal(eng.tap(_lib.SGM_TAP_COST, H, W), t["C"]) and np.array_equal(eng.tap(_lib.SGM_TAP_AGGR, H, W), t["S"])

    for eng, D, (H, W) in ((narrow, 256, A), (wide, 1024, A), (narrow, 256, A), (wide, 1024, B), (wide, 1024, A), (narrow, 256, A)):
        run(eng, D, H, W)
    m = cv.StereoSGBM_create(**case[256, 30][2])
    for D in (256, 1024, 256):
        m.setNumDisparities(D)
        assert np.array_equal(m.compute(*case[D, 30][:2]), case[D, 30][3]), D
    try:
        wide.set_option(_lib.SGM_OPT_POISON, 0xA5)    # fills every buffer the engine owns and arms the same for new ones
        run(wide, 1024, *B)
        wide.set_option(_lib.SGM_OPT_POISON, 0xA5)
        run(wide, 1024, *A)
        fresh = Engine(case[1024, 30][2])             # an engine whose buffers are born poisoned
        assert np.array_equal(fresh.compute_host(*case[1024, 30][:2]), case[1024, 30][3])
    finally:
        wide.set_option(_lib.SGM_OPT_POISON, -1)


# ---- guarded allocator (child process: a memory access fault ends the process that caused it) ------------------------------
def test_wide_rows_with_every_buffer_guarded():
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wide_guard_child.py")], capture_output=True, text=True, env=env,
                       timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"WIDE_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) == 6, tail
