"""Odd mid-size frames through the AUTOMATIC plan, every mode, bit for bit against the oracles.

make_plan (csrc/sgm_engine.hip) decides a good part of the schedule from the frame size: rows per band of k_box_u8 (RBb),
the row chunks of the fused pre-pass, the band height R of the sweeps, the chained window, the small-D schedule.  On the
tiny frames of the other GPU tests those decisions always take the same value; on the BASELINE frames of
test_gpu_configs.py they meet one friendly set of arguments and shapes without tails.  The cases here are the frames in
between -- 1013 x 2051, minDisparity -5, D = 192 -- with no option set but SGM_OPT_SCHEDULE (and SGM_OPT_KEEP_AGGR where
the volumes are compared): the plan a user gets.

Which plan a case takes is READ (_lib.debug_plan, csrc/sgm_debug.h), not assumed: every row states the plan it is in the
table for, and two tests that need no GPU hold the readout against the rows and against the coverage statement of
DESIGN.md 4.10, so the table cannot rot silently when make_plan changes.

Yardsticks: gray pairs in modes 0 and 1 -- the frozen oracle (oracle/sgbm_oracle.c); MODE_HH4 and colour pairs -- the
volume oracle (oracle/sgbm_volume_oracle.c, pinned by tests/test_volume_oracle.py).  Every comparison is exact.  No case
is skipped: every row must be inside the int16 regime and more than half valid from the oracle alone, and the tests assert
both.  Arguments: plain penalties P1 = 8 bs^2, P2 = 32 bs^2, speckle 60 / 2.

Measured on an MI355X box: see DESIGN.md 4.10."""
import functools
from collections import namedtuple

import numpy as np
import pytest

import bruteforce_color as BC
import parity_util as U
from oracle import oracle as O
from oracle import volume_oracle as V
from stereo_reconstruction_cv_amd import _lib, synth

Case = namedtuple("Case", "H W D minD bs mode cap uniq d12 sched cn plan")
MODE_NAME = {0: "SGBM", 1: "HH", 3: "HH4"}


def case(H, W, D, minD, bs, mode, cap=63, uniq=10, d12=1, sched=1, cn=1, **plan):
    return Case(H, W, D, minD, bs, mode, cap, uniq, d12, sched, cn, tuple(sorted(plan.items())))


def case_id(c):
    return f"{c.H}x{c.W} D{c.D} minD{c.minD} bs{c.bs} {MODE_NAME[c.mode]}{' colour' if c.cn == 3 else ''} sched{c.sched}"


# `plan`: what the row is in the table for, as fields of the readout; last_band / last_box / last_chunk are the rows of the
# last sweep band, of the last band of k_box_u8 and of the last pre-pass chunk
GRAY = [
    case(431, 1933, 192, -5, 9, 1, 31, 15, 1, W1=1741, R=4, last_band=3, RBb=96, fused_prepass=1, pre_nch=3, pre_rows=144, last_chunk=143),
    case(1013, 2051, 128, 7, 3, 0, 63, 10, 2, W1=1916, R=5, last_band=3, RBb=96, fused_prepass=1, pre_nch=8, pre_rows=128, last_chunk=117, nvol=2),
    case(1407, 2213, 256, 0, 5, 1, 15, 5, 1, W1=1957, R=8, last_band=7, RBb=96, pre_nch=10, pre_rows=144, last_chunk=111, NP=2, partial=0),
    case(1999, 2377, 320, -9, 7, 1, W1=2057, R=10, last_band=9, RBb=96, pre_nch=15, pre_rows=136, last_chunk=95, NP=4, partial=1),
    case(1605, 1891, 160, 0, 7, 0, W1=1731, R=7, last_band=2, RBb=96, pre_nch=12, pre_rows=136, last_chunk=109, fused_wta=1, path_w_main=1),
    case(389, 2999, 512, 0, 5, 0, W1=2487, R=4, last_band=1, RBb=96, pre_nch=3, pre_rows=136, last_chunk=117, NP=4, partial=0),
    case(150, 1801, 128, 0, 7, 1, W1=1673, R=4, last_band=2, RBb=48, last_box=6, pre_nch=1),
    case(95, 1801, 96, -2, 3, 0, W1=1705, R=4, last_band=3, RBb=32, last_box=31, pre_nch=1, NP=1, partial=1),
    case(611, 1777, 48, -3, 5, 0, 40, W1=1729, rows4=1, GWs=32, partial=1, RBb=96, nvol=5),
    case(517, 1699, 32, 3, 11, 1, 63, 0, -1, W1=1664, rows4=1, GWs=16, RBb=48, last_box=37),
    case(1081, 1921, 128, 0, 13, 1, 100, W1=1793, R=6, last_band=1, byte_cost=0, vsum_ring=0),
    case(707, 1931, 224, 4, 7, 1, sched=2, W1=1703, chain=1, R=12, last_band=11),
    case(1211, 2111, 64, -6, 5, 1, sched=2, W1=2047, chain=1, R=12, last_band=11, GWs=32),
    case(903, 1803, 384, 0, 3, 0, sched=2, W1=1419, chain=1, R=12, last_band=3, NP=4, partial=1),
    # added for the coverage statement: automatic R = 9 and 11 with a ragged last band, even W, the small-D schedule at
    # D = 16 and 64 on a wide frame
    case(1613, 1789, 96, 0, 5, 1, W1=1693, R=9, last_band=2, RBb=96, pre_nch=12, pre_rows=136, last_chunk=117),
    case(2003, 1700, 96, -4, 5, 1, W1=1604, R=11, last_band=1, RBb=96, pre_nch=15, pre_rows=136, last_chunk=99),
    case(333, 1811, 16, 0, 5, 0, W1=1795, rows4=1, GWs=8, nvol=5, RBb=16, last_box=13),
    case(455, 1902, 64, -1, 5, 1, W1=1838, rows4=1, GWs=32, partial=0, RBb=96),
]
# MODE_HH4: schedules 0, 1, 2; minDisparity < 0; D <= 64 (all four directions in one launch, nvol = 4)
HH4 = [
    case(431, 1933, 192, -5, 7, 3, 31, 15, 1, W1=1741, R=4, last_band=3, NP=2, partial=1),
    case(1013, 2051, 128, 7, 3, 3, 63, 10, 2, sched=0, W1=1916),
    case(707, 1931, 224, 4, 7, 3, sched=2, W1=1703, chain=1, R=12, last_band=11),
    case(611, 1777, 48, -3, 5, 3, 40, W1=1729, rows4=1, nvol=4, partial=1),
    case(150, 1801, 128, 0, 7, 3, W1=1673, R=4, last_band=2, RBb=48),
]
# colour pairs (the int16 cost pipeline: k_features<3>, k_hsum<., ., 3>): modes 0, 1, 3; schedules 1 and 2; D <= 32 and D = 192
COLOUR = [
    case(431, 1933, 192, -5, 5, 1, 31, 15, 1, cn=3, W1=1741, byte_cost=0, R=4, last_band=3, pre_nch=3, last_chunk=143),
    case(517, 1699, 32, 3, 5, 0, cn=3, W1=1664, byte_cost=0, pix_px=0, rows4=1, GWs=16, nvol=5),
    case(707, 1931, 128, 4, 7, 3, sched=2, cn=3, W1=1799, byte_cost=0, chain=1, R=12, last_band=11),
    case(1013, 2051, 128, 7, 3, 0, 63, 10, 2, sched=2, cn=3, W1=1916, byte_cost=0, chain=1, R=12, last_band=5),
]
ALL = GRAY + HH4 + COLOUR
FULL_HD = case(1080, 1920, 256, 0, 7, 3, W1=1664, NP=2, partial=0, R=6, RBb=96)   # (its own test at the end of the file)
ids = lambda cs: [case_id(c) for c in cs]


def params(c):
    return dict(minDisparity=c.minD, numDisparities=c.D, blockSize=c.bs, P1=8 * c.bs * c.bs, P2=32 * c.bs * c.bs,
                disp12MaxDiff=c.d12, preFilterCap=c.cap, uniquenessRatio=c.uniq, speckleWindowSize=60, speckleRange=2, mode=c.mode)


def readout(c, frames=1):
    q = _lib.debug_plan(params(c), c.H, c.W, c.cn, c.sched, frames=frames)
    q["last_band"] = c.H - (q["nbands"] - 1) * q["R"]
    q["last_box"] = c.H - (-(-c.H // q["RBb"]) - 1) * q["RBb"]
    q["last_chunk"] = c.H - (q["pre_nch"] - 1) * q["pre_rows"]
    return q


# ---- the table against the plan readout: no GPU ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL + [FULL_HD], ids=ids(ALL + [FULL_HD]))
def test_row_takes_the_plan_it_is_in_the_table_for(c):
    q = readout(c)
    want = dict(c.plan)
    assert {k: q[k] for k in want} == want, q
    assert q["W1"] > 0 and q["speckle"] == 1


def test_plan_coverage_of_the_table():
    """The coverage statement of DESIGN.md 4.10, from the readout over the whole table.  `sweeps`: rows that run the fused
    sweeps with the automatic band height (not chained, not the small-D schedule, not schedule 0)."""
    Q = [(c, readout(c)) for c in ALL]
    sweeps = [(c, q) for c, q in Q if c.sched == 1 and not q["rows4"] and not q["chain"]]
    # k_box_u8: 96, 48 and 32 rows per band, each with a last band that is not full
    for rbb in (96, 48, 32):
        assert any(q["byte_cost"] and q["RBb"] == rbb and c.H % rbb for c, q in Q), rbb
    # automatic band heights 4 .. 11, each with a ragged last band
    for R in range(4, 12):
        assert any(q["R"] == R and c.H % R for c, q in sweeps), R
    # the chained schedule: automatic R = 12 with a ragged last band, one and two passes, gray and colour, axis-only
    chained = [(c, q) for c, q in Q if q["chain"]]
    assert all(q["R"] == 12 and c.H % 12 for c, q in chained)
    assert {c.mode for c, _ in chained} == {0, 1, 3} and {c.cn for c, _ in chained} == {1, 3}
    # the fused pre-pass in at least three chunks with a short last one, for one- and two-pass modes
    for mode in (0, 1):
        assert any(c.mode == mode and q["fused_prepass"] and q["pre_nch"] >= 3 and 0 < q["last_chunk"] < q["pre_rows"]
                   for c, q in sweeps), mode
    assert all(q["pre_rows"] % 8 == 0 for _, q in Q)
    # shapes: odd and even W, odd W1, a first valid column that is no multiple of 4
    assert {c.W % 2 for c in ALL} == {0, 1}
    assert any(q["W1"] % 2 for _, q in Q) and any(q["minX1"] % 4 for _, q in Q)
    # NP = 1, 2, 4, each with and without the PARTIAL instantiation, on frames wider than 1536 valid columns
    wide = [(c, q) for c, q in Q if q["W1"] > 1536 and not q["rows4"]]
    assert {(q["NP"], q["partial"]) for _, q in wide} == {(n, part) for n in (1, 2, 4) for part in (0, 1)}
    # the small-D schedule at D = 16, 32, 48, 64 on such frames; D = 48 is the PARTIAL lane group
    small = {c.D: q for c, q in Q if q["rows4"] and q["W1"] > 1536 and c.cn == 1 and c.mode != 3}
    assert sorted(small) == [16, 32, 48, 64] and [small[d]["GWs"] for d in (16, 32, 48, 64)] == [8, 16, 32, 32]
    assert small[48]["partial"] == 1 and small[64]["partial"] == 0
    # winner-take-all: inside the last path kernel and as its own pass over 1, 2, 4 and 5 volumes
    assert {q["nvol"] for _, q in Q} == {1, 2, 4, 5} and {q["fused_wta"] for _, q in Q} == {0, 1}
    # both cost pipelines; the int16 one for a window above 11 x 11 (generic vertical sum) and for colour
    assert any(not q["byte_cost"] and not q["vsum_ring"] for _, q in Q) and any(c.cn == 3 and not q["byte_cost"] for c, q in Q)
    # MODE_HH4 in schedules 0, 1, 2, with minDisparity < 0, and in the small-D schedule
    assert {c.sched for c in HH4} == {0, 1, 2} and any(c.minD < 0 for c in HH4) and any(dict(c.plan).get("nvol") == 4 for c in HH4)
    assert {c.mode for c in COLOUR} == {0, 1, 3} and {c.sched for c in COLOUR} == {1, 2}
    assert any(c.D <= 32 for c in COLOUR) and any(c.D == 192 for c in COLOUR)


def test_chain_window_of_the_readout():
    """the automatic window of a chained launch: ceil(T / lag) workgroups per frame, T = ceil(W1 / pixels per step) +
    2 (R - 1) steps of a band and lag = 2 (R - 1) + 17 between a band and the one above, at most one per band and 256"""
    c = GRAY[11]
    q1, q5 = readout(c, 1), readout(c, 5)
    assert q1["chain"] and q1["nbands"] == 59
    assert 4 <= q1["chain_window"] <= q1["nbands"]
    assert q5["chain_window"] == min(5 * q1["chain_window"], 5 * q1["nbands"], 256)
    assert readout(GRAY[0])["chain_window"] == 0


# ---- inputs and oracle results ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair(c, k=0):
    """the pair of a row (k = 0), or another pair of its shape (the batches)"""
    if c.cn == 3:
        return BC.colour_pair(c.H, c.W, c.D, seed=4000 + c.H + 100 * k, minD=c.minD)
    return synth.make_pair(c.H, c.W, c.D, 4000 + c.H + 100 * k)[:2]


MAPS = ("disp_raw", "disp_median", "disp")
_light = {}


def _oracle(c, k, taps):
    l, r = pair(c, k)
    mod = O if c.cn == 1 and c.mode != 3 else V
    d, t = mod.sgbm_compute(l, r, taps=taps, **params(c))
    t["disp"] = d
    # the two conditions of every row, from the oracle alone: inside the int16 regime, and most of every map valid
    assert t["headroom_ok"], (case_id(c), k, t["max_cost_plus_p2"], t["max_delta"])
    for m in MAPS:
        assert (t[m] > (c.minD - 1) * 16).mean() > 0.5, (case_id(c), k, m)
    t["headroom"] = dict(ok=True, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"])
    _light[(c, k)] = {m: t[m] for m in MAPS + ("headroom",)}
    return t


def oracle_full(c):
    """every tap (not kept: the volumes of the table would add up to tens of GB); leaves the maps and the record behind"""
    return _oracle(c, 0, True)


def oracle_light(c, k=0):
    """maps and headroom record, computed once per session"""
    if (c, k) not in _light:
        _oracle(c, k, "light")
    return _light[(c, k)]


def say(c, what):
    """the case, before every compute: the last line of the output names what was running"""
    print(f"[midsize] {case_id(c)}: {what}", flush=True)


def engine(c, keep):
    from stereo_reconstruction_cv_amd.stereo import Engine
    eng = Engine(params(c))
    eng.set_option(_lib.SGM_OPT_SCHEDULE, c.sched)
    if keep:
        eng.set_option(_lib.SGM_OPT_KEEP_AGGR, 1)
    return eng


def run(eng, c, l, r, keep):
    disp = eng.compute_host(l, r)
    if c.sched == 2:
        eng.check()
    H, W = l.shape[:2]
    out = dict(disp=disp, disp_raw=eng.tap(_lib.SGM_TAP_DISP_RAW, H, W), disp_median=eng.tap(_lib.SGM_TAP_DISP_MEDIAN, H, W))
    if keep:
        out["C"] = eng.tap(_lib.SGM_TAP_COST, H, W)
        out["S"] = eng.tap(_lib.SGM_TAP_AGGR, H, W)
    out["headroom"] = eng.headroom()
    return out


def mismatches(h, t, keys):
    return [U.describe_mismatch(k, h[k], t[k]) for k in keys if not (h[k] == t[k] if k == "headroom" else np.array_equal(h[k], t[k]))]


# three rows also run once more after a frame of another shape went through the same engine (buffers regrown / reused)
AFTER_ANOTHER_SHAPE = {GRAY[0], GRAY[8], HH4[2]}


# ---- every row, every tap -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", ALL, ids=ids(ALL))
def test_every_tap(c):
    t = oracle_full(c)
    l, r = pair(c)
    keys = ("C", "S") + MAPS + ("headroom",)
    eng = engine(c, keep=True)
    for rep in range(2):         # twice on the same engine: buffer reuse
        say(c, f"compute {rep}, every tap")
        bad = mismatches(run(eng, c, l, r, True), t, keys)
        assert not bad, f"{case_id(c)} run {rep}:\n" + "\n".join(bad)
    if c in AFTER_ANOTHER_SHAPE:
        H2, W2 = 77, c.D + abs(c.minD) + 333
        other = pair(c._replace(H=H2, W=W2))
        say(c, f"a frame of {H2} x {W2}, then the row's again")
        eng.compute_host(*other)
        if c.sched == 2:
            eng.check()
        bad = mismatches(run(eng, c, l, r, True), t, keys)
        assert not bad, f"{case_id(c)} after another shape:\n" + "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("c", ALL, ids=ids(ALL))
def test_maps_without_keep_aggr(c):
    """SGM_OPT_KEEP_AGGR is a switch the kernels see (the last path kernel also stores S): a fresh engine with nothing set
    but the schedule"""
    t = oracle_light(c)
    say(c, "compute on a fresh engine, no option but the schedule")
    bad = mismatches(run(engine(c, keep=False), c, *pair(c), False), t, MAPS + ("headroom",))
    assert not bad, f"{case_id(c)}:\n" + "\n".join(bad)


# ---- the readout agrees with what ran -----------------------------------------------------------------------------------------
PROFILED = [GRAY[0], GRAY[1], GRAY[8], GRAY[10], GRAY[11], HH4[0], HH4[3], COLOUR[0], COLOUR[3]]


@pytest.mark.gpu
@pytest.mark.parametrize("c", PROFILED, ids=ids(PROFILED))
def test_stage_names_and_launch_counts_follow_the_readout(c):
    q = readout(c)
    eng = engine(c, keep=False)
    eng.set_option(_lib.SGM_OPT_PROFILE, 1)
    say(c, "profiled compute")
    got = eng.compute_host(*pair(c))
    eng.synchronize()
    stages = {n: k for n, _, k in eng.stage_times()}
    assert np.array_equal(got, oracle_light(c)["disp"])
    npass = 1 if c.mode == 0 else 2
    want = {"features_c3" if c.cn == 3 else "features": 1}
    want.update({"cost_pix": 1, "cost_box": 1} if q["byte_cost"] else {"cost_hsum_c3" if c.cn == 3 else "cost_hsum": 1, "cost_vsum": 1})
    if q["nvol"] == 5:
        want["paths5"] = 1
    elif q["nvol"] == 4:
        want["paths4"] = 1
    elif q["chain"]:
        want.update({"chain_dn": 1, "chain_up": 1} if npass == 2 else {"chain_dn": 1})
    elif q["rows4"]:
        want.update(prepass_dn=1, prepass_up=1, sweep_dn=1, sweep_up=1)
    else:
        chunks = q["pre_nch"] if q["fused_prepass"] else 1
        want.update(prepass_dn=chunks, sweep_dn=1)
        if npass == 2:
            want.update(prepass_up=chunks, sweep_up=1)
    if q["nvol"] in (2, 3):
        want["path_W"] = 1
    if q["path_w_main"]:
        want["path_W_wta" if q["fused_wta"] else "path_W"] = 1
    if not q["fused_wta"]:
        want["wta"] = 1
    for name, k in want.items():
        assert stages.get(name) == k, (name, k, stages)
    for name in ("prepass_dn", "prepass_up", "sweep_dn", "sweep_up", "sweep_up_wta", "chain_dn", "chain_up", "paths4", "paths5",
                 "cost_pix", "cost_box", "cost_hsum", "cost_hsum_c3", "cost_vsum", "wta", "path_W", "path_W_wta"):
        assert (name in stages) == (name in want), (name, stages)


# ---- batch entries at odd shapes ----------------------------------------------------------------------------------------------
BATCH = [GRAY[11], HH4[2], COLOUR[0]._replace(sched=2)]
BN = 5


def check_xyz(got, ref):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), "non-finite masks differ"
    assert np.array_equal(got[fin], ref[fin])


@pytest.mark.gpu
@pytest.mark.parametrize("gmax", [2, 0])
@pytest.mark.parametrize("c", BATCH, ids=ids(BATCH))
def test_resident_batch_of_different_pairs(c, gmax):
    """sgm_pipeline_batch_device, schedule 2, five different pairs of one odd shape: one chained launch per pass for a group
    (groups of 2, 2 and the last pair alone; or all five), int16 map, float map and XYZ of every pair"""
    import torch
    q = readout(c, BN)
    assert q["chain"] and c.H % q["R"] and q["chain_window"] > readout(c, 1)["chain_window"]
    want = [oracle_light(c, k) for k in range(BN)]
    Q = synth.default_Q(c.W)
    dev = torch.device("cuda", 0)
    pairs = [pair(c, k) for k in range(BN)]
    dl = [torch.from_numpy(a).to(dev) for a, _ in pairs]
    dr = [torch.from_numpy(b).to(dev) for _, b in pairs]
    dd = [torch.full((c.H, c.W), -7, dtype=torch.int16, device=dev) for _ in range(BN)]
    df = [torch.empty((c.H, c.W), dtype=torch.float32, device=dev) for _ in range(BN)]
    dx = [torch.empty((c.H, c.W, 3), dtype=torch.float32, device=dev) for _ in range(BN)]
    torch.cuda.synchronize()
    eng = engine(c, keep=False)
    eng.set_option(_lib.SGM_OPT_GROUP_MAX, gmax)
    ptr = lambda ts: [t.data_ptr() for t in ts]
    for rep in range(2):
        say(c, f"resident batch of {BN}, group max {gmax}, call {rep}")
        eng.pipeline_batch_device(ptr(dl), ptr(dr), c.H, c.W, c.W * c.cn, Q, ptr(dd), ptr(df), ptr(dx), cn=c.cn)
        eng.synchronize()
        eng.check()
        for k in range(BN):
            got = dd[k].cpu().numpy()
            assert np.array_equal(got, want[k]["disp"]), (rep, k, U.describe_mismatch("disp", got, want[k]["disp"]))
            f = O.disp_to_float(want[k]["disp"])
            assert np.array_equal(df[k].cpu().numpy().view(np.uint32), f.view(np.uint32)), (rep, k)
            check_xyz(dx[k].cpu().numpy(), O.reproject(f, Q))
        assert eng.headroom() == dict(ok=True, max_cost_plus_p2=max(w["headroom"]["max_cost_plus_p2"] for w in want),
                                      max_delta=max(w["headroom"]["max_delta"] for w in want)), eng.headroom()


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", [1, 2])
def test_host_batch_of_different_pairs(schedule):
    """sgm_compute_batch from host memory, both schedules, with Q"""
    c = BATCH[0]._replace(sched=schedule)
    want = [oracle_light(BATCH[0], k) for k in range(BN)]
    Q = synth.default_Q(c.W)
    pairs = [pair(BATCH[0], k) for k in range(BN)]
    eng = engine(c, keep=False)
    say(c, f"host batch of {BN}")
    disps, xyz = eng.compute_batch_host(np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]), Q)
    eng.check()
    for k in range(BN):
        assert np.array_equal(disps[k], want[k]["disp"]), (k, U.describe_mismatch("disp", disps[k], want[k]["disp"]))
        check_xyz(xyz[k], O.reproject(O.disp_to_float(want[k]["disp"]), Q))
    assert eng.headroom()["ok"]


# ---- MODE_HH4 at 1080p, D = 256 -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("schedule", [0, 1, 2])
def test_hh4_full_hd_against_the_volume_oracle(schedule):
    """1920 x 1080, D = 256, MODE_HH4: the map and the headroom record of every schedule against the volume oracle.
    (test_gpu_hh4.py::test_full_size_consistency holds the final map at 4K D = 256 against the same oracle; here the raw and
    the median map are compared too, per schedule, on a fresh engine each.)"""
    c = FULL_HD._replace(sched=schedule)
    t = oracle_light(FULL_HD)
    say(c, "compute")
    bad = mismatches(run(engine(c, keep=False), c, *pair(FULL_HD), False), t, MAPS + ("headroom",))
    assert not bad, "\n".join(bad)
