"""The clamped and biased path state of the chained sweeps on the GPU (csrc/kernels_path.h: path_elem<.., BIAS>; the
arithmetic is pinned without a GPU by tests/test_path_bias_reference.py).  k_sweep_chain and k_axis_chain hold every path
state -- in registers, in the LDS rings, in the hand-off record the bands pass through HBM -- as min(L, P2) + (32767 - P2);
nothing a caller can read is in that form, so every tap and the headroom record must equal the oracle's, bit for bit, in
throughput mode (schedule 2).  MODE_HH4 is compared with its numpy restatement (tests/bruteforce_hh4.py: the C oracle
refuses mode 3), as tests/test_gpu_hh4.py does.  Shapes are the smallest that still have two bands, a guarded tail block
and, per case, the lane packing named beside it."""
import numpy as np
import pytest

import bruteforce_hh4 as HH4
import parity_util as U
from oracle import oracle as O
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu

STAGES = ("C", "S", "disp_raw", "disp_median", "disp")
_PAIRS = {}


def _pair(H, W, D, seed=31):
    if (H, W, D, seed) not in _PAIRS:
        _PAIRS[(H, W, D, seed)] = synth.make_pair(H, W, D, seed)[:2]
    return _PAIRS[(H, W, D, seed)]


def _params(D, mode, **kw):
    return U.params(D, 5, 0, mode, speckleWindowSize=30, speckleRange=2, **kw)


def _check(l, r, p, sweep_rows=0, chain_wgs=0, chained=True):
    """every tap and the headroom record of one compute in throughput mode against the oracle (mode 3: the restatement)"""
    H, W = l.shape
    plan = _lib.debug_plan(p, H, W, schedule=2, sweep_rows=sweep_rows)
    assert plan["chain"] == int(chained), plan        # which kernels run is read, not assumed
    if p["mode"] == 3:
        w = HH4.sgbm_hh4(l, r, **p)
        _, t = O.sgbm_compute(l, r, taps=True, **dict(p, mode=1))
        assert t["max_cost_plus_p2"] <= 32767 and w["max_delta"] <= 32767, "case left the int16 regime"
        h = U.run_hip_with_taps(l, r, p, 2, sweep_rows, chain_wgs=chain_wgs)
        bad = [U.describe_mismatch(k, h[k], w[k]) for k in STAGES if not np.array_equal(h[k], w[k])]
        hr = dict(ok=True, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=w["max_delta"])
        if h["headroom"] != hr:
            bad.append(f"headroom record: hip {h['headroom']} != {hr}")
        assert not bad, "\n".join(bad)
        return h
    rep, t, h = U.compare_stages(l, r, p, schedule=2, sweep_rows=sweep_rows, chain_wgs=chain_wgs)
    assert t["headroom"]["ok"], "case left the int16 regime"
    assert set(STAGES) | {"headroom"} <= set(rep), rep
    bad = [U.describe_mismatch(k, h[k], t[k]) for k, n in rep.items() if n]
    assert not bad, "\n".join(bad)
    return h


# lane packings: NP 1 full / NP 2 full / NP 2 partial / NP 1 partial / NP 4 / lane groups (D <= 64: two and four pixels
# per wave in the in-row kernels, whose state stays unbiased beside the chained sweep's)
PACKINGS = [(14, 200, 128), (14, 330, 256), (12, 270, 192), (12, 160, 80), (8, 600, 512), (14, 120, 64), (14, 100, 48)]


@pytest.mark.parametrize("mode", [0, 1, 3])
@pytest.mark.parametrize("H,W,D", PACKINGS)
def test_every_lane_packing_and_kernel(H, W, D, mode):
    l, r = _pair(H, W, D)
    # frames of at most 12 rows are one band of the automatic plan and would not be chained: bands of 3 (8 rows: 3 + 3 + 2,
    # the last with a row past the image) and of 5 (12 rows: 5 + 5 + 2)
    rows = {8: 3, 12: 5}.get(H, 0)
    h = _check(l, r, _params(D, mode), sweep_rows=rows)
    assert (h["disp"][:, D:] >= 0).mean() > 0.05, "degenerate case"


@pytest.mark.parametrize("rows,wgs", [(1, 1), (12, 0)])
@pytest.mark.parametrize("H,W,D", [(14, 200, 128), (14, 330, 256)])
@pytest.mark.parametrize("mode", [1, 3])
def test_hand_off_through_the_record(H, W, D, mode, rows, wgs):
    """bands of one row on one workgroup: every row's state goes through the HBM record and comes back biased; bands of
    twelve rows: through the LDS rings eleven times, then the record"""
    l, r = _pair(H, W, D)
    _check(l, r, _params(D, mode), sweep_rows=rows, chain_wgs=wgs)


@pytest.mark.parametrize("W1", [1, 7, 8, 9, 16, 17])
@pytest.mark.parametrize("D", [128, 256])
def test_row_ends(D, W1):
    """rows of W1 matched columns: tail-only rows, and the virtual pixel W1 (the biased start state) in every ring slot"""
    H, W = 5, D + W1
    l, r = _pair(H, W, D, seed=40 + W1)
    for mode in (1, 3):
        _check(l, r, _params(D, mode), sweep_rows=2)


def _largest_p2_inside(l, r, D):
    """the largest P2 for which the oracle still reports the int16 regime: from the record at a small P2, then down"""
    p = _params(D, 1)
    _, t = O.sgbm_compute(l, r, taps=True, **p)
    P2 = 32767 - max(t["max_cost_plus_p2"] - p["P2"], t["max_delta"] - p["P2"])
    for _ in range(64):
        _, t = O.sgbm_compute(l, r, taps=True, **dict(p, P2=P2))
        if t["headroom_ok"]:
            return P2
        P2 -= max(1, max(t["max_cost_plus_p2"], t["max_delta"]) - 32767)
    raise AssertionError("no P2 inside the regime found")


@pytest.mark.parametrize("which", ["p2_is_p1_plus_1", "p1_is_1", "p1_is_p2_minus_1", "largest_p2"])
@pytest.mark.parametrize("H,W,D", [(14, 200, 128), (14, 330, 256)])
def test_penalties_inside_the_regime(H, W, D, which):
    l, r = _pair(H, W, D)
    base = _params(D, 1)
    if which == "p2_is_p1_plus_1":
        kw = dict(P2=base["P1"] + 1)
    elif which == "p1_is_1":
        kw = dict(P1=1)
    elif which == "p1_is_p2_minus_1":
        kw = dict(P1=base["P2"] - 1)
    else:
        kw = dict(P2=_largest_p2_inside(l, r, D))
        print(f"D = {D}: largest P2 inside the regime {kw['P2']} (bias {32767 - kw['P2']})")
        assert kw["P2"] > base["P2"]
    h = _check(l, r, dict(base, **kw))          # (asserts the oracle's headroom_ok)
    assert h["headroom"]["ok"]


@pytest.mark.parametrize("P2", [32767, 40000])
@pytest.mark.parametrize("H,W,D", [(14, 200, 128), (14, 330, 256)])
def test_outside_the_regime_the_engine_returns_and_says_so(H, W, D, P2):
    """P2 + any cost > 32767: no int16 form of the recurrence is exact and no map is compared.  The bias is
    max(0, 32767 - P2) = 0; the engine returns and its headroom record says `ok = False`, as the oracle's does."""
    l, r = _pair(H, W, D)
    p = dict(_params(D, 1), P2=P2)
    _, t = O.sgbm_compute(l, r, taps=True, **p)
    assert not t["headroom_ok"]
    h = U.run_hip_with_taps(l, r, p, 2)
    assert h["headroom"]["ok"] is False, h["headroom"]
    assert h["disp"].shape == (H, W)


@pytest.mark.parametrize("D", [256, 128])
def test_batch_entry_with_the_reducing_sweep(D):
    """three different pairs through sgm_pipeline_batch_device: the second chained pass is the SWEEP_REDUCE form (no S kept),
    maps, float maps and XYZ of every pair against the oracle's for that pair"""
    import torch
    H, W, N = 40, 300, 3
    p = _params(D, 1)
    assert _lib.debug_wta_split(p, H, W)
    Q = synth.default_Q(W)
    pairs = [_pair(H, W, D, seed=6100 + i) for i in range(N)]
    dev = torch.device("cuda", 0)
    dl = [torch.from_numpy(a).to(dev) for a, _ in pairs]
    dr = [torch.from_numpy(b).to(dev) for _, b in pairs]
    dd = [torch.full((H, W), -7, dtype=torch.int16, device=dev) for _ in range(N)]
    df = [torch.empty((H, W), dtype=torch.float32, device=dev) for _ in range(N)]
    dx = [torch.empty((H, W, 3), dtype=torch.float32, device=dev) for _ in range(N)]
    torch.cuda.synchronize()
    ptr = lambda ts: [t.data_ptr() for t in ts]
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, 2)
    eng.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, Q, ptr(dd), ptr(df), ptr(dx))
    eng.synchronize()
    oracle = [O.sgbm_compute(a, b, taps=True, **p) for a, b in pairs]
    for i, (want, t) in enumerate(oracle):
        got = dd[i].cpu().numpy()
        assert np.array_equal(got, want), (i, int((got != want).sum()))
        wf = np.ascontiguousarray(O.disp_to_float(want), np.float32)
        assert np.array_equal(df[i].cpu().numpy().view(np.uint32), wf.view(np.uint32)), i
        ref = O.reproject(wf, Q)
        fin = np.isfinite(ref)
        x = dx[i].cpu().numpy()
        assert np.array_equal(np.isfinite(x), fin) and np.array_equal(x[fin], ref[fin]), i
    hr = eng.headroom()
    assert hr == dict(ok=all(t["headroom_ok"] for _, t in oracle), max_cost_plus_p2=max(t["max_cost_plus_p2"] for _, t in oracle),
                      max_delta=max(t["max_delta"] for _, t in oracle)), hr
