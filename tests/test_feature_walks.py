"""What tests/test_gpu_feature_walk.py rests on, checked without a GPU: the conditions that keep the feature walks
(tests/feature_walk.py) from hiding a failure.  They are decided by the references and by the plan readouts of the library
alone (sgm_debug_plan*, sgm_debug_wta_split: which plan a step takes is read, not assumed)."""
import numpy as np
import pytest

import feature_walk as FW
import history_walk as HW

DEVICE_ENTRIES = ("compute_device", "pipeline_device", "pipeline_batch_device")
SINGLE_ENTRIES = ("compute_host", "compute_device", "pipeline_device")
NVOL = dict(sgbm_d32={2, 3, 5}, sgbm_d64_c3={1, 2, 5}, hh4_d48_c3={1, 4})


def walk_problems(index, steps):
    """what a walk lacks of the per-walk coverage, as a list of sentences (empty: nothing).  Needs no reference."""
    name, p, colour, _ = FW.ENGINES[index]
    bad = []
    need = lambda ok, what: None if ok else bad.append(f"{name}: {what}")
    need(len(steps) == FW.STEPS, "16 steps")
    need({s["opts"]["schedule"] for s in steps} == {0, 1, 2}, "schedules 0, 1, 2")
    need(len({s["entry"] for s in steps}) >= 4, "four entry points")
    need({s["opts"]["cost"] for s in steps} == {FW.BT, FW.CENSUS}, "both cost functions")
    need(all(s["cn"] == 1 for s in steps if s["opts"]["cost"] == FW.CENSUS), "census on gray steps only")
    need({(s["opts"]["confidence"], s["opts"]["right_view"]) for s in steps} == {(0, 0), (0, 1), (1, 0), (1, 1)}, "the four (confidence, right view)")
    for opt, flag in (("confidence", "bind_conf"), ("right_view", "bind_right")):
        on = [s for s in steps if s["opts"][opt]]
        need(all(s["entry"] in DEVICE_ENTRIES for s in steps if s[flag]), f"{opt}: bound on device entries only")
        need(not any(s[flag] for s in steps if not s["opts"][opt]), f"{opt}: bound only where it is on")
        if on:
            need(any(s[flag] for s in on), f"{opt}: a step with a bound map")
            need(any(not s[flag] and s["entry"] in SINGLE_ENTRIES for s in on), f"{opt}: a step with a tapped map")
    w1 = [FW.width1(p, s["W"]) for s in steps]
    need(min(w1) <= 2 and max(w1) >= 150, f"W1 from nothing to wide: {min(w1)} .. {max(w1)}")
    need(all(1 <= s["H"] <= 48 and (w <= 0 or s["H"] * w * p["numDisparities"] <= FW.VOL_CAP) for s, w in zip(steps, w1)), "the shape caps")
    shapes = [(s["H"], s["W"]) for s in steps]
    grows = sum(1 for x, y in zip(shapes, shapes[1:]) if y[0] * y[1] > x[0] * x[1])
    need(3 <= grows <= len(steps) - 4, f"grows and shrinks: {grows}")
    need(not any(s["opts"]["debug"] & 64 for s in steps), "never bit 64")
    need(any(s["replay"] for s in steps), "a replayed frame")
    need(all(s["n"] == 1 or "batch" in s["entry"] for s in steps) and all(1 <= s["n"] <= 3 for s in steps), "1..3 pairs on the batch entries")
    if colour:
        need({s["cn"] for s in steps} == {1, 3}, "both channel counts")
        need(sum(s["between"] == "refuse" for s in steps) == 1, "one refuse")
    else:
        need(all(s["cn"] == 1 for s in steps) and not any(s["between"] == "refuse" for s in steps), "gray only")
    if name in NVOL:          # the volume counts of the small-D schedules: which engine is to reach which
        nv = {q["nvol"] for q in (FW.plan_of(p, s) for s in steps) if q is not None}
        need(nv >= NVOL[name], f"winner-take-all over {sorted(NVOL[name])} volumes: {sorted(nv)}")
    if name in ("hh_d128", "hh_d256"):
        sp = [q["wta_split"] for q in (FW.plan_of(p, s) for s in steps) if q is not None]
        pairs = set(zip(sp, sp[1:]))
        need((False, True) in pairs and (True, False) in pairs, f"the split winner-take-all switched on and off: {sp}")
    return bad


WALKS = FW.all_walks()


def test_walks_are_reproducible_and_replayable():
    for i, (name, p, steps) in enumerate(WALKS):
        assert FW.make_walk(i) == steps == FW.make_walk(i), name
        assert FW.make_walk(i, seed=FW.ENGINES[i][3]) == steps
        assert eval(repr(steps)) == steps, name            # the step list a failure message prints IS the walk
    assert [e[0] for e in FW.ENGINES] == ["sgbm_d32", "sgbm_d64_c3", "sgbm_d160", "hh_d128", "hh_d256", "hh4_d48_c3", "hh4_d528", "hh_d1024"]


@pytest.mark.parametrize("index", range(len(FW.ENGINES)), ids=FW.NAMES)
def test_coverage_of_each_walk(index):
    assert not walk_problems(index, WALKS[index][2])


def test_coverage_over_all_walks_together():
    steps = [s for _, _, w in WALKS for s in w]
    kinds = {s["between"] for s in steps}
    assert kinds == set(FW.ALL_CALLS) and set(HW.BETWEEN) <= kinds, sorted(set(FW.ALL_CALLS) - kinds)
    for kind in FW.HOST_AND_DEVICE:
        assert {s["bdev"] for s in steps if s["between"] == kind} == {False, True}, kind
    for bit in FW.NEW_DEBUG_BITS:
        assert any(s["opts"]["debug"] & (7 << 17 if bit == FW.WLS_ROWS else 3 << 20 if bit == FW.WLS_COLS else bit) == bit for s in steps), bit
    # ... each on a step whose call it acts on
    for kind, bits in FW.OF_CALL.items():
        for bit in {b for v in bits for b in FW.NEW_DEBUG_BITS if v & b}:
            assert any(s["opts"]["debug"] & bit for s in steps if s["between"] == kind), (kind, bit)
    assert {s["bopt"]["nb_neighbors"] for s in steps if s["between"] == "statistical"} == set(FW.NB_NEIGHBORS)
    assert {s["bopt"]["radius"] for s in steps if s["between"] in ("lrc", "lrc_batch")} == {0, 3, 16}
    assert {s["bopt"]["max_diff"] for s in steps if "mesh" in s["between"] or s["between"] == "normals"} == set(FW.MAX_DIFF)
    assert {s["bopt"]["layered"] for s in steps if s["between"] in ("voxel", "radius", "statistical")} == {False, True}
    assert {s["bopt"]["n"] for s in steps if s["between"] in ("wls_batch", "lrc_batch")} == {1, 2, 3}
    for s in steps:
        b = s["bopt"]
        if s["between"] in ("voxel", "radius", "statistical"):
            assert 0.01 <= b["radius"] <= 0.05 and b["n"] <= 6000 and b["H"] <= 48 and b["W"] <= 320
        if s["between"] in ("wls", "wls_batch"):
            assert b["H"] <= 70 and b["W"] <= 260


def test_the_plans_the_walks_reach():
    """read with sgm_debug_plan* and sgm_debug_wta_split"""
    plans = [[FW.plan_of(p, s) for s in w] for _, p, w in WALKS]
    seq = lambda name, f: [q[f] for q in plans[FW.NAMES.index(name)] if q is not None]
    split = set()
    for name in ("hh_d128", "hh_d256"):
        sp = seq(name, "wta_split")
        split |= set(zip(sp, sp[1:]))
    assert {(False, True), (True, False)} <= split, split
    fused = set()
    for name in FW.NAMES:
        f = seq(name, "fused_wta")
        fused |= set(zip(f, f[1:]))
    assert {(0, 1), (1, 0)} <= fused, fused
    assert {q["nvol"] for w in plans for q in w if q is not None} >= {1, 2, 3, 4, 5}
    assert set(seq("hh_d1024", "NP")) == {8} == set(seq("hh4_d528", "NP")) and 8 not in set(seq("hh_d256", "NP"))     # D > 512
    # both box routes under both cost functions, and the split select beside a confidence map's own winner-take-all
    assert {(q["byte_cost"], s["opts"]["cost"]) for (_, _, w), qs in zip(WALKS, plans) for s, q in zip(w, qs) if q is not None} == \
        {(0, FW.BT), (1, FW.BT), (0, FW.CENSUS), (1, FW.CENSUS)}


def _mixed(a, invalid):
    return bool((a == invalid).any() and (a != invalid).any())


@pytest.mark.parametrize("index", range(len(FW.ENGINES)), ids=FW.NAMES)
def test_regime_and_degeneracy_of_each_walk(index):
    """At most one step in eight leaves the int16 regime (such a step is not compared on the GPU, only the engine's verdict
    is); the compared ones have something to compare; a cost or a channel switch the engine ignored would show."""
    name, p, steps = WALKS[index]
    inv = (p["minDisparity"] - 1) * 16
    out = [s["k"] for s in steps if not FW.step_ok(p, s)]
    assert 8 * len(out) <= len(steps), (name, out)
    wide = [s for s in steps if s["k"] not in out and FW.width1(p, s["W"]) >= 32]
    assert len(wide) >= 4, name
    assert 2 * sum(_mixed(FW.expected(p, s)["disp"], inv) for s in wide) >= len(wide), name
    rv = [s for s in wide if s["opts"]["right_view"]]
    # (the right view of plain noise at D = 1024 is invalid everywhere: every matchable step must have both, of all steps half)
    assert rv and all(_mixed(FW.expected_maps(p, s)["right"], inv) for s in rv if not s["noise"]), name
    assert 2 * sum(_mixed(FW.expected_maps(p, s)["right"], inv) for s in rv) >= len(rv), name
    cf = [s for s in wide if s["opts"]["confidence"]]
    assert cf and all(len(np.unique(FW.expected_maps(p, s)["conf_raw"])) >= 3 for s in cf), name
    # the maps of a step without a volume are the pinned ones
    for s in steps:
        if FW.width1(p, s["W"]) <= 0:
            m = FW.expected_maps(p, s)
            assert all((m[k] == 0).all() for k in ("conf_raw", "conf") if k in m) and all((m[k] == inv).all() for k in ("right_raw", "right") if k in m)
    # an ignored flip would show
    census = [s for s in wide if s["opts"]["cost"] == FW.CENSUS]
    assert any(not np.array_equal(FW.expected(p, s)["disp"], FW.expected(p, s, cost=FW.BT)["disp"]) for s in census), name
    if FW.ENGINES[index][2]:
        def first_channel(s):
            l, r = FW.pair(p, s)
            d, _ = FW.V.sgbm_compute(np.ascontiguousarray(l[..., 0]), np.ascontiguousarray(r[..., 0]), taps="light", **p)
            return d
        colour = [s for s in wide if s["cn"] == 3]
        assert any(not np.array_equal(FW.expected(p, s)["disp"], first_channel(s)) for s in colour), name


def test_the_hand_written_sequences_change_the_plan_under_one_frame():
    for name in FW.NAMES:
        p, steps = FW.ENGINES[FW.NAMES.index(name)][1], FW.sequence_same_frame_other_plan(name)
        assert bool(steps) == (name in ("hh_d128", "sgbm_d64_c3"))
        if not steps:
            continue
        assert len({(s["H"], s["W"]) for s in steps}) == 1 and all(FW.step_ok(p, s) for s in steps), name
        assert len({s["seed"] for s in steps}) == len(steps)          # another input every time: a stale result would show
        plans = [FW.plan_of(p, s) for s in steps]
        batch = [q for s, q in zip(steps, plans) if s["n"] > 1]
        assert len(batch) >= 8 and all(q["chain"] for s, q in zip(steps, plans) if s["opts"]["schedule"] == 2), name
        assert {q["byte_cost"] for q in batch} == {0, 1}, name
        if name == "hh_d128":
            sp = [q["wta_split"] for q in plans]
            assert {(True, False), (False, True)} <= set(zip(sp, sp[1:])) and sp[0] and sp[-1], sp
        else:
            assert {q["nvol"] for q in plans} == {1, 2, 3, 5} and {s["cn"] for s in steps} == {1, 3}, name
            assert any(s["opts"]["debug"] == 2 | 2048 for s in steps)


def test_the_references_of_the_calls_compose():
    """every kind of call in front of a compute: its inputs build and its reference answers, on the first step that has it"""
    seen = {}
    for _, _, w in WALKS:
        for s in w:
            seen.setdefault(s["between"], s)
    for kind, s in seen.items():
        x = FW.call_input(s)
        want = FW.call_want(s, x)
        assert (want is None) == (kind in HW.BETWEEN or kind == "refuse"), kind
