"""What tests/test_gpu_cloud_walk.py rests on, checked without a GPU: the conditions that keep the cloud walks
(tests/cloud_walk.py) from hiding a failure.  They are decided by the references alone: if one fails for a seed, look for another
seed, do not loosen the condition."""
import numpy as np
import pytest

import cloud_walk as CW
import feature_walk as FW
import icp_ref as IR

WALKS = CW.all_walks()
N = len(CW.ENGINES)


def wants(index):
    """[(step, inputs, reference)] of a walk's steps that have a cloud (cached in cloud_walk)"""
    out = []
    for s in WALKS[index][2]:
        if s["cloud"] is not None:
            x = CW.call_input(s)
            out.append((s, x, CW.call_want(s, x)))
    return out


def capacities(index):
    """[(step, slots of its table)] of the grid users of a walk, in order"""
    return [(s, CW.capacity(s, w)) for s, _, w in wants(index) if s["kind"] in CW.GRID_USERS]


def test_walks_are_reproducible_and_replayable():
    for i, (name, p, steps) in enumerate(WALKS):
        assert CW.make_walk(i) == steps == CW.make_walk(i), name
        assert CW.make_walk(i, seed=CW.ENGINES[i][3]) == steps
        assert eval(repr(steps)) == steps, name            # the step list a failure message prints IS the walk
        assert [s["k"] for s in steps] == list(range(CW.STEPS))
    assert CW.NAMES == ["sgbm_d32", "sgbm_d64_c3", "hh_d128", "hh4_d48_c3"]
    assert [e[2] for e in CW.ENGINES] == [False, True, False, True]
    assert all(CW.sequence_behind_the_walk(name) == [] for name in CW.NAMES)      # (no walk has found a failure to keep covered)


@pytest.mark.parametrize("index", range(N), ids=CW.NAMES)
def test_coverage_of_each_walk(index):
    name, p, steps = WALKS[index]
    kinds = [s["kind"] for s in steps]
    assert len(steps) == CW.STEPS == 24
    assert set(CW.NEW_KINDS) | set(CW.EVENTS) <= set(kinds), sorted(set(CW.NEW_KINDS) - set(kinds))
    assert {s["arg"]["est"] for s in steps if s["kind"] == "icp"} == {0, 1}
    assert len(set(kinds) & set(CW.OLD_KINDS)) >= 3, kinds
    assert kinds.count("refuse") == 1 and kinds.count("trim") == 1 and kinds.count("compute") == 1
    # seven of the 24 steps replay the cloud of the step before; a change of the radius or of the origin alone is among them
    rep = [s for s in steps if s["replay"]]
    assert len(rep) == 7 and {s["replay"] for s in rep} & {"radius", "origin"}
    for s in rep:
        b = steps[s["k"] - 1]
        assert {k: v for k, v in s["cloud"].items() if k != "empty"} == b["cloud"], s
        assert (s["kind"] != b["kind"]) == (s["replay"] == "kind")
        if s["replay"] != "kind":
            f = "origin" if s["replay"] == "origin" else "radius"
            assert {k: v for k, v in s["arg"].items() if k != f} == {k: v for k, v in b["arg"].items() if k != f} and s["arg"][f] != b["arg"][f]
            assert s["disp"] == b["disp"]
    # the volume: three frames, two extractions, other kinds between its steps, the last extraction behind the last frame
    vol = [s for s in steps if s["kind"].startswith("tsdf")]
    assert [s["kind"] for s in vol] == ["tsdf_integrate", "tsdf_integrate", "tsdf_extract", "tsdf_integrate", "tsdf_extract"]
    assert [s["arg"]["frame"] for s in vol if s["kind"] == "tsdf_integrate"] == [0, 1, 2]
    assert all(b["k"] - a["k"] >= 2 for a, b in zip(vol, vol[1:]))
    # the caps
    for s in steps:
        c, a = s["cloud"], s["arg"]
        if c is not None:
            pts = CW.points_of(c)
            assert (pts[0] <= CW.CAPS["ns"] and pts[1] <= CW.CAPS["nt"]) if c["gen"] == "pair" else pts[0] <= CW.CAPS["points"], s
        assert a.get("maxit", 0) <= CW.CAPS["max_iteration"] and a.get("K", 0) <= CW.CAPS["K"]
        assert s["debug"] & ~sum(CW.DEBUG_BITS) == 0
        if s["empty"] == "n0":
            assert not s["dev"]
    for a in CW.volume_frames(index):
        assert tuple(a["dims"]) == CW.CAPS["dims"] and a["xyz"].shape[0] <= 48 and a["xyz"].shape[1] <= 64
    # the compute is inside the int16 regime: no step of a walk is left uncompared
    for s in steps:
        if s["kind"] == "compute":
            f = CW.compute_step(p, s)
            assert FW.width1(p, f["W"]) >= 20 and FW.step_ok(p, f), f


@pytest.mark.parametrize("index", range(N), ids=CW.NAMES)
def test_tables_of_other_sizes_and_empty_clouds_behind_full_ones(index):
    caps = capacities(index)
    seq = [c for _, c in caps if c]
    assert len(set(seq)) >= 4, seq
    grows = sum(1 for a, b in zip(seq, seq[1:]) if b > a)
    shrinks = sum(1 for a, b in zip(seq, seq[1:]) if b < a)
    assert grows >= 3 and shrinks >= 3, seq
    # a cloud with nothing in range directly behind a call that filled the grid, and a grid user directly behind an empty one
    steps = WALKS[index][2]
    by_k = {s["k"]: c for s, c in caps}
    behind_full = [s for s, c in caps if c == 0 and by_k.get(s["k"] - 1, 0) > 0]
    behind_empty = [s for s, c in caps if c > 0 and by_k.get(s["k"] - 1, 1) == 0]
    assert len(behind_full) >= 2 and behind_empty, (behind_full, behind_empty)
    for s, c in caps:
        assert (c == 0) == (s["empty"] in ("origin", "disp", "nan", "n0")), (s, c)
        if s["empty"] == "n1":
            assert c in (1, 2)
    assert any(s["empty"] for s in steps)


def test_coverage_over_all_walks_together():
    steps = [s for _, _, w in WALKS for s in w]
    assert {s["kind"] for s in steps} == set(CW.ALL_KINDS)
    for kind in CW.HOST_AND_DEVICE:
        dev = {(s["arg"]["entry"] != "compute_host") if kind == "compute" else s["dev"] for s in steps if s["kind"] == kind}
        assert dev == {False, True}, kind
    # every debug bit meets the call it acts on, the tight table every grid user
    for kind, bits in (("covariance", (CW.SEP, CW.SEL)), ("dbscan", (CW.GATHER,)), ("plane", (CW.OTHER,))):
        for bit in bits:
            assert any(s["debug"] & bit for s in steps if s["kind"] == kind), (kind, bit)
    for kind in CW.GRID_USERS:
        assert any(s["debug"] & CW.TIGHT and s["empty"] is None for s in steps if s["kind"] == kind), kind
    # ... and each grid user an empty cloud directly behind a full grid
    empty_behind_full = set()
    for i in range(N):
        caps = capacities(i)
        by_k = {s["k"]: c for s, c in caps}
        empty_behind_full |= {s["kind"] for s, c in caps if c == 0 and by_k.get(s["k"] - 1, 0) > 0}
    assert empty_behind_full == set(CW.GRID_USERS), empty_behind_full
    assert {s["empty"] for s in steps} >= {"origin", "disp", "nan", "n0", "n1"}
    tr = [s for s in steps if s["kind"] == "transform"]
    assert {s["arg"]["normals"] for s in tr} == {False, True}
    assert {(s["dev"], s["arg"]["alias"]) for s in tr} >= {(True, True), (True, False), (False, False)}
    # the stages only one route has: a profiled step on that route
    assert any(s["profile"] and s["debug"] & CW.SEP for s in steps if s["kind"] == "covariance")
    assert any(s["profile"] and s["arg"]["refine"] for s in steps if s["kind"] == "plane")
    for kind in CW.STAGES:
        assert any(s["profile"] and s["empty"] is None for s in steps if s["kind"] == kind), kind
        assert any(not s["profile"] for s in steps if s["kind"] == kind), kind
    # which optional outputs are null
    for kind, names in CW.OUTS.items():
        asked = [s["outs"] for s in steps if s["kind"] == kind]
        assert names in asked and any(len(o) < len(names) for o in asked), kind
    status = {int(CW.call_want(s, CW.call_input(s))["stats"][7]) for s in steps if s["kind"] == "icp"}
    assert len(status) >= 2 and status <= {IR.CONVERGED, IR.MAX_ITER, IR.TOO_FEW, IR.DEGENERATE}, status


_degenerate, _no_partner = [], []


@pytest.mark.parametrize("index", range(N), ids=CW.NAMES)
def test_the_steps_of_each_walk_have_something_to_compare(index):
    w = wants(index)
    of = lambda kind: [(s, r) for s, _, r in w if s["kind"] == kind]
    # clusters with border and noise points
    assert any(int(r["stats"][5]) >= 2 and int(r["stats"][3]) > 0 and int(r["stats"][4]) > 0 for _, r in of("dbscan")), [r["stats"] for _, r in of("dbscan")]
    # a plane that is found and holds between a tenth and nine tenths of the valid points
    assert any(int(r["stats"][7]) == 1 and 0.1 * int(r["stats"][0]) <= r["n_inliers"] <= 0.9 * int(r["stats"][0]) for _, r in of("plane"))
    assert all(0 < r["n_inliers"] and 0 < r["n_selected"] < s["cloud"]["H"] * s["cloud"]["W"] for s, r in of("plane_inliers"))
    cov = of("covariance")
    assert 2 * sum(int(r["stats"][2]) > 0 for _, r in cov) >= len(cov)
    _degenerate.extend(int(r["stats"][3]) for _, r in cov)
    icp = of("icp") + of("evaluate")
    assert 2 * sum(int(r["stats"][4]) > 0 for _, r in icp) >= len(icp)
    _no_partner.extend(int(r["stats"][4]) == 0 for _, r in icp)
    for s, r in of("radius"):
        assert s["empty"] or 0 < r["n_kept"]
    for s, r in of("voxel"):
        assert 0 < r["n_voxels"] < CW.points_of(s["cloud"])[0]
    # the volume: its weights reach 3, and the last extraction is a cloud
    vol = CW.volume_wants(index, WALKS[index][2])
    last_i = max(k for k, v in vol.items() if WALKS[index][2][k]["kind"] == "tsdf_integrate")
    last_e = max(k for k, v in vol.items() if WALKS[index][2][k]["kind"] == "tsdf_extract")
    assert last_e > last_i and vol[last_i][0][1].max() == 3 and vol[last_e][0].shape[0] > 100
    assert (vol[last_e][1] is not None) == (CW.volume_frames(index)[0]["colors"] is not None)


def test_degenerate_neighbourhoods_and_sources_without_a_partner_occur():
    """(over all walks; behind the per-walk test, which collects them)"""
    assert len(_degenerate) >= N and any(d > 0 for d in _degenerate), _degenerate
    assert any(_no_partner)


def _differs(a, b):
    if isinstance(a, dict):
        return any(_differs(a[k], b[k]) for k in a if k in b and k not in ("sums", "P"))
    if a is None or b is None:
        return (a is None) != (b is None)
    a, b = np.asarray(a), np.asarray(b)
    return a.shape != b.shape or a.tobytes() != b.tobytes()


@pytest.mark.parametrize("index", range(N), ids=CW.NAMES)
def test_an_ignored_change_of_the_radius_or_the_origin_would_show(index):
    steps = WALKS[index][2]
    seen = 0
    for s in steps:
        if s["replay"] in ("radius", "origin"):
            f = s["replay"]
            x = CW.call_input(s)
            stale = CW.call_want(s, x, **{f: steps[s["k"] - 1]["arg"][f]})
            assert _differs(CW.call_want(s, x), stale), s
            seen += 1
    assert seen >= 1


def test_the_references_of_the_calls_compose():
    """every kind of call: its inputs build and its reference answers, on the first step that has it"""
    seen = {}
    for i, (_, _, w) in enumerate(WALKS):
        for s in w:
            seen.setdefault(s["kind"], (i, s))
    assert set(seen) == set(CW.ALL_KINDS)
    for kind, (i, s) in seen.items():
        x = CW.call_input(s)
        want = CW.call_want(s, x)
        if kind.startswith("tsdf"):
            assert s["k"] in CW.volume_wants(i, WALKS[i][2])
        else:
            assert (want is None) == (kind in CW.EVENTS), kind
