"""MODE_HH4 on the GPU (needs an MI355X): the MODE_HH pipeline over the four axis-aligned paths, through the axis-only
kernels (k_axis_sweep, k_axis_chain, k_axis_prepass; k_axis_paths4_g for D <= 64; k_path per direction in schedule 0).
The yardstick is the numpy restatement tests/bruteforce_hh4.py (the C oracle refuses mode 3); every comparison is
bit-exact over the whole frame.  The full-size test compares the schedules and the batch entry with each other and with the
volume oracle (oracle/sgbm_volume_oracle.c: the C form of the restatement, pinned by tests/test_volume_oracle.py), which
reaches 4K where the numpy helper cannot."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bruteforce_color as BC
import bruteforce_hh4 as HH4
import parity_util as U
from oracle import oracle as O
from oracle import volume_oracle as V
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd import stereo as cv
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [  # H, W, D, bs, minD, penalty
    (24, 72, 16, 3, 0, "plain"), (30, 100, 32, 5, 0, "plain"), (40, 150, 64, 5, -8, "plain"), (64, 200, 48, 3, 5, "plain"),
    (37, 211, 128, 7, 0, "notebook"), (33, 330, 256, 7, 0, "notebook"), (135, 240, 16, 11, 0, "notebook"),
    (96, 480, 128, 7, 0, "notebook"), (23, 900, 512, 5, 0, "plain"),
]
TALL = (270, 640, 128, 5, 0, "notebook")
_want = {}


def want_for(case):
    """the helper's stages for a case (cached: the schedules of a case share it) and the oracle's cost-stage record"""
    if case not in _want:
        H, W, D, bs, minD, penalty = case
        l, r, _ = synth.make_pair(H, W, D, seed=11)
        p = U.params(D, bs, minD, 3, penalty=penalty)
        w = HH4.sgbm_hh4(l, r, **p)
        _, t = O.sgbm_compute(l, r, taps=True, **dict(p, mode=1))
        assert np.array_equal(w["C"], t["C"])
        w["max_cost_plus_p2"] = t["max_cost_plus_p2"]
        assert w["max_cost_plus_p2"] <= 32767 and w["max_delta"] <= 32767, "case left the int16 regime"
        _want[case] = (l, r, p, w)
    return _want[case]


def check_stages(case, schedule, sweep_rows=0, prepass_rows=0, chain_wgs=0):
    l, r, p, w = want_for(case)
    h = U.run_hip_with_taps(l, r, p, schedule, sweep_rows, prepass_rows=prepass_rows, chain_wgs=chain_wgs)
    bad = [U.describe_mismatch(k, h[k], w[k]) for k in ("C", "S", "disp_raw", "disp_median", "disp") if not np.array_equal(h[k], w[k])]
    hr = dict(ok=True, max_cost_plus_p2=w["max_cost_plus_p2"], max_delta=w["max_delta"])
    if h["headroom"] != hr:
        bad.append(f"headroom record: hip {h['headroom']} != {hr}")
    assert not bad, f"{case} schedule {schedule} rows {sweep_rows}: " + "\n".join(bad)
    return h


@pytest.mark.parametrize("schedule", [0, 1, 2])
@pytest.mark.parametrize("case", CASES)
def test_every_stage_against_the_restatement(case, schedule):
    h = check_stages(case, schedule)
    valid = (h["disp"] > (case[4] - 1) * 16).mean()
    assert 0.1 < valid < 0.95, valid


def test_result_is_neither_mode_hh_nor_mode_sgbm():
    l, r, p, w = want_for(CASES[7])
    for mode in (0, 1):
        other = O.sgbm_compute(l, r, **dict(p, mode=mode))
        assert (other != w["disp"]).mean() > 0.05, mode


@pytest.mark.parametrize("rows", [1, 2, 3, 5, 9, 10, 11])
@pytest.mark.parametrize("schedule", [1, 2])
def test_band_heights(schedule, rows):
    check_stages(CASES[7], schedule, sweep_rows=rows)


@pytest.mark.parametrize("wgs", [1, 2, 7, 64])
def test_chain_window_sizes(wgs):
    check_stages(CASES[7], 2, sweep_rows=5, chain_wgs=wgs)
    check_stages(CASES[7], 2, chain_wgs=wgs)


@pytest.mark.parametrize("chunk", [8, 40])
def test_prepass_rows_option_changes_nothing(chunk):
    """(the axis-only pre-pass is one column scan without chunks: the option must be accepted and leave the result alone)"""
    check_stages(CASES[7], 1, prepass_rows=chunk)


@pytest.mark.parametrize("schedule", [0, 1, 2])
def test_taller_frame_with_automatic_settings(schedule):
    check_stages(TALL, schedule)


@pytest.mark.parametrize("schedule", [0, 1, 2])
def test_colour_pair(schedule):
    H, W, D = 20, 160, 64
    p = U.params(D, 5, 0, 3, penalty="plain", speckleWindowSize=12, speckleRange=2)
    L3, R3 = BC.colour_pair(H, W, D, seed=77)
    w = HH4.sgbm_hh4(L3, R3, pixel_cost=BC.pixel_cost_c3, **p)
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, schedule)
    eng.set_option(_lib.SGM_OPT_KEEP_AGGR, 1)
    if schedule == 2:
        eng.set_option(_lib.SGM_OPT_SWEEP_ROWS, 3)
    got = eng.compute_host(L3, R3)
    assert eng.headroom()["ok"] and eng.headroom()["max_delta"] == w["max_delta"]
    assert np.array_equal(eng.tap(_lib.SGM_TAP_COST, H, W), w["C"])
    assert np.array_equal(eng.tap(_lib.SGM_TAP_AGGR, H, W), w["S"])
    assert np.array_equal(eng.tap(_lib.SGM_TAP_DISP_RAW, H, W), w["disp_raw"])
    assert np.array_equal(got, w["disp"])


# ---- batch entries -----------------------------------------------------------------------------------------------------
BH, BW, BD, BN = 96, 480, 128, 5


def _batch():
    p = U.params(BD, 7, 0, 3)
    pairs = [synth.make_pair(BH, BW, BD, seed=11 + i)[:2] for i in range(BN)]
    single = Engine(p)
    want = [single.compute_host(a, b) for a, b in pairs]
    assert np.array_equal(want[0], want_for(CASES[7])[3]["disp"])     # pair 0 is the case the helper covers
    return p, pairs, want


@pytest.mark.parametrize("gmax", [2, 0])
def test_batch_entries_in_throughput_mode(gmax):
    import torch
    p, pairs, want = _batch()
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, 2)
    eng.set_option(_lib.SGM_OPT_GROUP_MAX, gmax)
    disps = eng.compute_batch_host(np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]))
    for i in range(BN):
        assert np.array_equal(disps[i], want[i]), ("host", i, int((disps[i] != want[i]).sum()))
    dev = torch.device("cuda", 0)
    dl = [torch.from_numpy(a).to(dev) for a, _ in pairs]
    dr = [torch.from_numpy(b).to(dev) for _, b in pairs]
    dd = [torch.full((BH, BW), -7, dtype=torch.int16, device=dev) for _ in range(BN)]
    torch.cuda.synchronize()
    eng.pipeline_batch_device([t.data_ptr() for t in dl], [t.data_ptr() for t in dr], BH, BW, BW, None, [t.data_ptr() for t in dd])
    eng.synchronize()
    eng.check()
    for i in range(BN):
        assert np.array_equal(dd[i].cpu().numpy(), want[i]), ("device", i)
    assert eng.headroom()["ok"]


def test_dist_batch_compute_and_ingest_pipeline():
    import torch
    from stereo_reconstruction_cv_amd import dist as D_
    p, pairs, want = _batch()
    dev = torch.device("cuda", 0)
    l = torch.from_numpy(np.stack([a for a, _ in pairs]))
    r = torch.from_numpy(np.stack([b for _, b in pairs]))
    for schedule in (1, 2):
        out = D_.hip_batch_compute(p, schedule=schedule)(l.to(dev), r.to(dev))
        out = out[0] if isinstance(out, (tuple, list)) else out
        for i in range(BN):
            assert np.array_equal(out[i].cpu().numpy(), want[i]), (schedule, i)
    cs = torch.cuda.Stream(dev)
    compute = D_.hip_batch_compute(p, schedule=2, stream=cs, synchronize=False)
    pipe = D_.IngestPipeline(compute, src=0, device=dev, compute_stream=cs)
    for _ in range(2):
        pipe.step(l, r)
    for res in pipe.drain():
        disp = res[0] if isinstance(res, (tuple, list)) else res
        for i in range(BN):
            assert np.array_equal(disp[i].cpu().numpy(), want[i]), i


def test_stereo_sgbm_surface_and_neighbouring_modes():
    l, r, p, w = want_for(CASES[4])
    pm = dict(p)
    m = cv.StereoSGBM_create(**pm)
    assert m.getMode() == cv.STEREO_SGBM_MODE_HH4
    hh = cv.StereoSGBM_create(**dict(pm, mode=cv.STEREO_SGBM_MODE_HH))
    before = hh.compute(l, r)
    assert np.array_equal(before, O.sgbm_compute(l, r, **dict(pm, mode=1)))
    assert np.array_equal(m.compute(l, r), w["disp"])
    assert np.array_equal(hh.compute(l, r), before)          # a mode-1 compute before and after: unchanged
    with pytest.raises(cv.error, match="3WAY"):
        cv.StereoSGBM_create(**dict(pm, mode=cv.STEREO_SGBM_MODE_SGBM_3WAY)).compute(l, r)
    # the same on engines of their own, interleaved: HH4 -> HH -> HH4
    e3, e1 = Engine(pm), Engine(dict(pm, mode=1))
    a = e3.compute_host(l, r)
    b = e1.compute_host(l, r)
    assert np.array_equal(e3.compute_host(l, r), a) and np.array_equal(a, w["disp"]) and np.array_equal(b, before)


_want_4k = []


def volume_oracle_4k(l, r, p):
    """map and headroom record of the 4K pair from the volume oracle (about half a minute and 8 GB on one core), kept"""
    if not _want_4k:
        _want_4k.append(V.sgbm_compute(l, r, taps="light", **p))
    return _want_4k[0]


def test_full_size_consistency():
    """2160 x 3840, D = 256, bs = 7: schedules 0, 1, 2 and a throughput-mode batch of 3 give the same map and the same
    headroom record -- and they are the volume oracle's (the numpy restatement cannot reach this size; the C form of it can)."""
    H, W, D = 2160, 3840, 256
    p = U.params(D, 7, 0, 3)
    l, r, _ = synth.make_pair(H, W, D, seed=11)
    want, t = volume_oracle_4k(l, r, p)
    assert t["headroom_ok"] and (want >= 0).mean() > 0.5
    maps, hrs = [], []
    for schedule in (0, 1, 2):
        eng = Engine(p)
        eng.set_option(_lib.SGM_OPT_SCHEDULE, schedule)
        maps.append(eng.compute_host(l, r))
        hrs.append(eng.headroom())
        eng.check()
        del eng
    assert hrs[0]["ok"], hrs[0]
    assert hrs[0] == hrs[1] == hrs[2], hrs
    assert np.array_equal(maps[0], maps[1]) and np.array_equal(maps[0], maps[2])
    assert 0.3 < (maps[0] >= 0).mean() < 0.99
    hh = Engine(dict(p, mode=1)).compute_host(l, r)
    assert (hh != maps[0]).mean() > 0.02               # not MODE_HH under another name
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, 2)
    disps = eng.compute_batch_host(np.stack([l, l, l]), np.stack([r, r, r]))
    eng.check()
    for i in range(3):
        assert np.array_equal(disps[i], maps[0]), i
    assert eng.headroom() == hrs[0]
    assert hrs[0] == dict(ok=True, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"]), (hrs[0], t)
    assert np.array_equal(maps[0], want), U.describe_mismatch("disp", maps[0], want)


def test_small_cases_with_guarded_allocations():
    """the band record changes layout in this mode ([band][x][1][D]); with SGM_DEBUG_ALLOC=1 every buffer ends at the end
    of its mapping, so an index that leaves the record faults instead of reading a neighbour -- in a child process"""
    env = dict(os.environ, SGM_DEBUG_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hh4_guard_child.py")], capture_output=True, text=True, env=env, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"HH4_GUARD_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) == 3 * len(CASES), tail
