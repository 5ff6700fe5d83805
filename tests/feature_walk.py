"""Seeded walks of a long-lived engine through the PRODUCT of what the engine can be asked for, and what every step of them
must compute (no GPU needed).

tests/history_walk.py stopped at the engine as it was when it was written: gray or colour pairs, the BT cost, D <= 512, the
disparity map alone.  The walks here draw, on one living engine, everything that came since: numDisparities up to 1024, the
cost function, the confidence and the right-view option, where their maps go (the engine's taps, or caller tensors through
the bind entries), and in front of every compute one of the stand-alone calls that share the engine's buffers with it (the
edge-aware filter, the left-right confidence, the voxel grid, the two outlier filters, the mesh and the normals).  One step in
three REPLAYS the shape of the step before it with one or two options flipped: the case in which an engine finds its buffers
sized for the frame and must notice that the plan now wants more of them.

Shared by tests/feature_walk_child.py (which takes the walks on the GPU) and tests/test_feature_walks.py (which regenerates
them with the references alone and checks the conditions that keep them meaningful).  Everything is a function of (engine
index, walk seed): a failing walk can be replayed from the step list its failure message prints.  The point-cloud calls added
later (covariance normals, clustering, planes, registration, the TSDF volume) are walked in tests/cloud_walk.py."""
from __future__ import annotations

import numpy as np

import census_ref as CE
import confidence_ref as CR
import history_walk as HW
import lrc_ref as LR
import mesh_ref as MR
import normals_ref as NR
import parity_util as U
import radius_ref as RR
import right_view_ref as RV
import statistical_ref as SR
import voxel_ref as VR
import wls_ref as WR
from history_walk import DEBUG_BITS as OLD_DEBUG_BITS, ENTRIES, POISON, describe, pair, width1  # noqa: F401
from oracle import oracle as O
from oracle import volume_oracle as V
from stereo_reconstruction_cv_amd import _lib

SP = dict(speckleWindowSize=30, speckleRange=2)
# (name, parameters, 3-channel-capable, walk seed).  Every set stays inside the int16 regime for a matchable pair and for plain
# noise, under BT and under census, the two colour-capable ones for three channels as well.  The seeds are the first ones (from
# 31000 + 101 * index upwards) under which the walk meets the conditions of tests/test_feature_walks.py: if a change to the
# generator breaks one of them, look for another seed, do not loosen the condition.
ENGINES = [
    ("sgbm_d32", U.params(32, 7, 0, 0, **SP), False, 31014),
    ("sgbm_d64_c3", U.params(64, 3, -5, 0, penalty="plain", **SP), True, 31103),
    ("sgbm_d160", U.params(160, 5, 2, 0, **SP), False, 31202),
    ("hh_d128", U.params(128, 5, 0, 1, **SP), False, 31307),
    ("hh_d256", U.params(256, 7, 0, 1, **SP), False, 31408),
    ("hh4_d48_c3", U.params(48, 5, 3, 3, penalty="plain", **SP), True, 31509),
    ("hh4_d528", U.params(528, 3, 0, 3, **SP), False, 31606),
    ("hh_d1024", U.params(1024, 3, 0, 1, **SP), False, 31707),
]
NAMES = [e[0] for e in ENGINES]
STEPS = 16
VOL_CAP = 1_200_000         # elements of one pair's cost volume: H * W1 * D
BT, CENSUS = _lib.SGM_COST_BT, _lib.SGM_COST_CENSUS

# SGM_OPT_DEBUG values whose results stay bit-exact (csrc/sgm_debug.h; never 64): those of the history walks, the A/B bits of the
# point-cloud calls, and one non-zero value of each of the edge-aware filter's two shape fields
WLS_ROWS, WLS_COLS = 2 << 17, 2 << 20
NEW_DEBUG_BITS = (_lib.SGM_DBG_VOXEL_TIGHT_TABLE, _lib.SGM_DBG_VOXEL_OTHER_REDUCTION, _lib.SGM_DBG_RADIUS_TIGHT_TABLE,
                  _lib.SGM_DBG_RADIUS_SOURCE_ORDER, _lib.SGM_DBG_STAT_WIDE_LIST, WLS_ROWS, WLS_COLS)
DEBUG_BITS = tuple(OLD_DEBUG_BITS) + NEW_DEBUG_BITS
# ... and the ones that mean something to the call in front of the compute: walk `index` adds OF_CALL[kind][index % 4] on the
# step of that call, so that every one of them meets its call whatever the general draw gives
_VT, _VO, _RT, _RS, _SW = NEW_DEBUG_BITS[:5]
OF_CALL = dict(voxel=(0, _VT, _VO, _VT | _VO), radius=(_RT, _RS, _RT | _RS, 0), statistical=(_SW, _RT, 0, _SW | _RT),
               wls=(WLS_ROWS, WLS_COLS, 0, WLS_ROWS | WLS_COLS), wls_batch=(0, WLS_ROWS | WLS_COLS, WLS_ROWS, WLS_COLS))

NB_NEIGHBORS = (1, 8, 9, 16, 33, 64)        # every list capacity of k_stat_query
MAX_DIFF = (0.125, 1.0, 100.0)
# the calls in front of a compute.  NEW: each occurs once in every walk; of the history walks' own (HW.BETWEEN) five are drawn
# beside them; `refuse` takes the place of one of those on the colour-capable engines.
NEW_CALLS = ("wls", "wls_batch", "lrc", "lrc_batch", "voxel", "radius", "statistical", "mesh", "normals", "mesh_normals", "trim")
HOST_AND_DEVICE = ("wls", "wls_batch", "lrc", "voxel", "radius", "statistical", "mesh", "normals", "mesh_normals")
ALL_CALLS = tuple(dict.fromkeys(HW.BETWEEN + NEW_CALLS + ("refuse",)))


def _draw_call(rng, kind, index):
    """the arguments of the call in front of a compute: sizes that have nothing to do with the compute"""
    ri = lambda lo, hi: int(rng.integers(lo, hi + 1))
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]
    if kind in ("wls", "wls_batch"):
        return dict(n=1 if kind == "wls" else ri(1, 3), H=ri(1, 70), W=ri(1, 260), cn=pick((1, 3)), with_conf=bool(ri(0, 1)),
                    lam=pick((100.0, 8000.0)), sigma=pick((0.5, 1.5, 10.0)), invalid=pick((-16, -160)))
    if kind in ("lrc", "lrc_batch"):
        return dict(n=1 if kind == "lrc" else ri(1, 3), H=ri(1, 48), W=ri(1, 330), radius=pick((0, 3, 16)), with_base=bool(ri(0, 1)))
    if kind in ("voxel", "radius", "statistical"):
        b = dict(layered=bool(ri(0, 1)), H=ri(1, 48), W=ri(1, 320), n=ri(1, 6000), radius=round(float(rng.uniform(0.01, 0.05)), 4),
                 with_colors=bool(ri(0, 1)))
        if kind == "voxel":
            b["min_points"] = pick((1, 2))
        elif kind == "radius":
            b["nb_points"] = pick((1, 4, 8))
        else:
            # (the walks' indices run through the six capacities; the draw moves the ones behind them)
            b.update(nb_neighbors=NB_NEIGHBORS[(index + (ri(0, 1) if index >= len(NB_NEIGHBORS) else 0)) % len(NB_NEIGHBORS)],
                     std_ratio=pick((0.5, 1.0, 2.0)))
        return b
    if kind in ("mesh", "normals", "mesh_normals"):
        return dict(H=ri(1, 48), W=ri(1, 320), max_diff=pick(MAX_DIFF), orient=ri(0, 1), with_colors=bool(ri(0, 1)))
    return {}


def make_walk(index: int, seed: int | None = None, steps: int = STEPS):
    """The steps of engine ENGINES[index]'s walk: a list of plain dicts."""
    name, p, colour, wseed = ENGINES[index]
    rng = np.random.default_rng(wseed if seed is None else seed)
    D, minD = p["numDisparities"], p["minDisparity"]
    edge = max(minD + D, 0) - min(minD, 0)      # the width at which W1 = 0
    calls = list(NEW_CALLS) + [HW.BETWEEN[int(j)] for j in rng.integers(0, len(HW.BETWEEN), steps - len(NEW_CALLS))]
    if colour:
        calls[-1] = "refuse"
    calls = [calls[int(j)] for j in rng.permutation(len(calls))][:steps]
    bound = dict(confidence=bool(index % 2), right_view=not index % 2)       # where the next map of a device entry goes
    out, prev = [], None
    for k in range(steps):
        sliver = k % 7 == 3
        replay = prev is not None and k % 3 == 1 and not sliver
        if replay:
            H, W, cn = prev["H"], prev["W"], prev["cn"]
        else:
            cn = 3 if colour and rng.integers(0, 2) else 1
            W = int(rng.integers(max(2, edge - 10), edge + 3)) if sliver else int(edge + rng.integers(1, 261))
            H = int(rng.integers(1, 49))
            W1 = width1(p, W)
            if W1 > 0:
                H = max(1, min(H, VOL_CAP // (W1 * D)))
        entry = ENTRIES[int(rng.integers(0, len(ENTRIES)))]
        n = int(rng.integers(1, 4)) if "batch" in entry else 1
        nbits = int(rng.integers(0, 3)) * int(rng.integers(0, 2))   # half of the steps: no debug bit; else one or two
        debug = 0
        for b in rng.choice(len(DEBUG_BITS), nbits, replace=False):
            debug |= DEBUG_BITS[int(b)]
        fresh = dict(schedule=int(rng.integers(0, 3)), sweep_rows=int(rng.choice([0, 0, 1, 2, 3, 5, 9])),
                     prepass_rows=int(rng.choice([0, 0, 3, 11, 64])), chain_wgs=int(rng.choice([0, 1, 2, 7])),
                     group_max=int(rng.choice([0, 1, 2])), keep_aggr=int(rng.integers(0, 2)), profile=int(rng.integers(0, 2)),
                     debug=debug, cost=CENSUS if cn == 1 and rng.integers(0, 3) == 0 else BT,
                     confidence=int(rng.integers(0, 2)), right_view=int(rng.integers(0, 2)))
        if replay:
            # the frame of the step before, one or two options flipped: the buffers are sized, the plan is another
            opts = dict(prev["opts"], profile=fresh["profile"])
            for f in rng.choice(["confidence", "right_view", "keep_aggr", "cost", "schedule", "debug"], int(rng.integers(1, 3)), replace=False):
                if f in ("confidence", "right_view", "keep_aggr"):
                    opts[f] = 1 - opts[f]
                elif f == "cost":
                    opts[f] = (CENSUS if opts[f] == BT else BT) if cn == 1 else BT
                elif f == "schedule":
                    opts[f] = (opts[f] + 1 + int(rng.integers(0, 2))) % 3
                else:
                    opts[f] = debug
        else:
            opts = fresh
        call = calls[k]
        # the bits that belong to the call of the step before go; this call's come
        opts["debug"] = (opts["debug"] & ~sum(NEW_DEBUG_BITS) | (debug & sum(NEW_DEBUG_BITS))) | OF_CALL.get(call, (0,) * 4)[index % 4]
        binds = {}
        for o in ("confidence", "right_view"):
            binds[o] = False
            if opts[o] and entry in ("compute_device", "pipeline_device", "pipeline_batch_device"):
                binds[o] = bound[o]
                bound[o] = not bound[o]
        s = dict(k=k, H=H, W=W, cn=cn, noise=(k % 5 == 4), seed=int(rng.integers(0, 10 ** 6)), entry=entry, n=n,
                 with_q=bool(rng.integers(0, 2)), pad=int(rng.integers(1, 40)), replay=replay,
                 bind_conf=binds["confidence"], bind_right=binds["right_view"],
                 between=call, bdev=bool((k + index) % 2), bseed=int(rng.integers(0, 10 ** 6)), bopt=_draw_call(rng, call, index),
                 opts=opts)
        out.append(s)
        prev = s
    return out


def step(H, W, seed=1, entry="compute_host", n=1, cn=1, noise=False, with_q=True, pad=7, between="none", bdev=False, bseed=3,
         bopt=None, bind_conf=False, bind_right=False, **opts):
    """A hand-written step (for a named sequence that keeps a found failure covered whatever the seeds become)."""
    o = dict(schedule=1, sweep_rows=0, prepass_rows=0, chain_wgs=0, group_max=0, keep_aggr=1, profile=1, debug=0, cost=BT,
             confidence=0, right_view=0)
    assert set(opts) <= set(o), opts
    o.update(opts)
    return dict(k=-1, H=H, W=W, cn=cn, noise=noise, seed=seed, entry=entry, n=n, with_q=with_q, pad=pad, replay=False,
                bind_conf=bind_conf, bind_right=bind_right, between=between, bdev=bdev, bseed=bseed, bopt=bopt or {}, opts=o)


# ---- what a compute must give --------------------------------------------------------------------------------------------------
_cache: dict = {}


def _key(p, s, i):
    return (tuple(sorted(p.items())), s["H"], s["W"], s["cn"], s["seed"], s["noise"], s["n"], i)


def expected(p, s, i=0, cost=None):
    """What pair i of step s must give under parameters p and the step's cost function (`cost`: that one instead):
    dict(disp, disp_raw, disp_median[, C, S], hr, ok).  hr is the headroom record; ok False: the input leaves the int16 regime
    and nothing but the engine's own verdict is compared.  Cached."""
    cost = s["opts"]["cost"] if cost is None else cost
    key = _key(p, s, i) + (cost,)
    if key in _cache:
        return _cache[key]
    l, r = pair(p, s, i)
    if cost == CENSUS:
        assert s["cn"] == 1
        t = CE.census_sgbm(l, r, **p)
        e = {k: np.asarray(t[k]).astype(np.int16) for k in ("disp", "disp_raw", "disp_median", "C", "S") if k in t}
        e.update(ok=bool(t["headroom"]["ok"]), hr=dict(t["headroom"]))
        if e["ok"]:
            assert all(np.array_equal(e[k], t[k]) for k in e if k not in ("ok", "hr"))       # (nothing was cut to 16 bits)
    else:
        if width1(p, s["W"]) <= 0 and l.ndim == 3:       # no volume at all: every pixel invalid whatever the channels
            l, r = np.ascontiguousarray(l[..., 0]), np.ascontiguousarray(r[..., 0])
        d, t = (V if p["mode"] == 3 or l.ndim == 3 else O).sgbm_compute(l, r, taps=True, **p)
        ok = bool(t["headroom_ok"])
        e = {k: t[k] for k in ("disp_raw", "disp_median", "C", "S") if k in t}
        e.update(disp=d, ok=ok, hr=dict(ok=ok, max_cost_plus_p2=int(t["max_cost_plus_p2"]), max_delta=int(t["max_delta"])))
    if "S" not in e:
        assert (e["disp"] == (p["minDisparity"] - 1) * 16).all()
    _cache[key] = e
    return e


def expected_maps(p, s, i=0):
    """The optional maps of pair i of step s, from the aggregated volume of expected(): dict(conf_raw, conf) where the step has
    SGM_OPT_CONFIDENCE on, dict(right_raw, right) where it has SGM_OPT_RIGHT_VIEW on.  Without a volume the confidence is 0
    everywhere (tests/test_gpu_confidence.py) and every right-view pixel invalid.  Cached."""
    o = s["opts"]
    key = _key(p, s, i) + (o["cost"], "maps", o["confidence"], o["right_view"])
    if key in _cache:
        return _cache[key]
    e = expected(p, s, i)
    H, W, minD = s["H"], s["W"], p["minDisparity"]
    minX1 = max(minD + p["numDisparities"], 0)
    m = {}
    if o["confidence"]:
        if "S" in e:
            m["conf_raw"] = CR.conf_raw(e["S"], W, minX1)
            m["conf"] = CR.conf_final(m["conf_raw"], e["disp"], minD)
        else:
            m["conf_raw"] = m["conf"] = np.zeros((H, W), np.uint8)
    if o["right_view"]:
        if "S" in e:
            m["right_raw"], m["right"] = RV.right_view(e["S"], W, minX1, p)
        else:
            m["right_raw"] = m["right"] = RV.all_invalid(H, W, minD)
    _cache[key] = m
    return m


def step_ok(p, s):
    return all(expected(p, s, i)["ok"] for i in range(s["n"]))


# ---- the calls in front of a compute: inputs and references ----------------------------------------------------------------------
def cloud(s):
    """(xyz, disp, colors) of a point-cloud call: lists for voxel / radius / statistical, an organised cloud for the mesh calls"""
    b, kind = s["bopt"], s["between"]
    if kind in ("mesh", "normals", "mesh_normals"):
        xyz, disp, col = VR.layered_cloud(b["H"], b["W"], s["bseed"])
    elif b["layered"]:
        xyz, disp, col = VR.layered_cloud(b["H"], b["W"], s["bseed"])
        xyz, disp, col = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)
    else:
        xyz, col = RR.random_list(b["n"], s["bseed"], extent=0.5)
        disp = None
    return np.ascontiguousarray(xyz), disp, (np.ascontiguousarray(col) if b["with_colors"] else None)


def call_input(s):
    """the inputs of step s's call: a dict (empty for the calls history_child.Runner.between builds itself)"""
    b, kind = s["bopt"], s["between"]
    if kind in ("wls", "wls_batch"):
        return dict(maps=[WR.random_input(b["H"], b["W"], b["cn"], s["bseed"] + j, b["invalid"], 0.3, b["with_conf"]) for j in range(b["n"])],
                    lut=WR.weights(b["sigma"]))
    if kind in ("lrc", "lrc_batch"):
        return dict(pairs=[LR.random_pair(b["H"], b["W"], s["bseed"] + j) for j in range(b["n"])])
    if kind in ("voxel", "radius", "statistical", "mesh", "normals", "mesh_normals"):
        return dict(zip(("xyz", "disp", "colors"), cloud(s)))
    return {}


def call_want(s, x):
    """the reference of step s's call on the inputs x = call_input(s)"""
    b, kind = s["bopt"], s["between"]
    if kind in ("wls", "wls_batch"):
        return [WR.wls_filter(m["disp"], m["guide"], m["conf"], b["invalid"], b["lam"], x["lut"]) for m in x["maps"]]
    if kind in ("lrc", "lrc_batch"):
        return [LR.lrc_confidence(q["dl"], q["dr"], q["base"] if b["with_base"] else None, -16, LR.T_DEFAULT, b["radius"], LR.V_DEFAULT)
                for q in x["pairs"]]
    if kind == "voxel":
        return VR.voxel_downsample(x["xyz"], x["disp"], x["colors"], b["radius"], (0.0, 0.0, 0.0), b["min_points"])
    if kind == "radius":
        return RR.cells(x["xyz"], x["disp"], x["colors"], b["radius"], b["nb_points"])
    if kind == "statistical":
        return SR.cells(x["xyz"], x["disp"], x["colors"], b["nb_neighbors"], b["std_ratio"], b["radius"])
    if kind == "mesh":
        return MR.mesh_grid(x["xyz"], x["disp"], x["colors"], b["max_diff"])
    if kind == "normals":
        return dict(image=NR.normal_image(x["xyz"], x["disp"], b["max_diff"], b["orient"]))
    if kind == "mesh_normals":
        return NR.mesh_grid_normals(x["xyz"], x["disp"], x["colors"], b["max_diff"], b["orient"])
    return None


# ---- the plans the steps take (read, not assumed; no GPU) ------------------------------------------------------------------------
def plan_of(p, s):
    """dict(wta_split, fused_wta, nvol, NP, ...) of the compute of step s, or None where the frame has no volume"""
    if width1(p, s["W"]) <= 0:
        return None
    o = s["opts"]
    q = _lib.debug_plan(p, s["H"], s["W"], s["cn"], o["schedule"], o["sweep_rows"], o["prepass_rows"], o["debug"], s["n"],
                        o["confidence"], o["right_view"], o["cost"])
    q["wta_split"] = _lib.debug_wta_split(p, s["H"], s["W"], o["schedule"], o["sweep_rows"], o["debug"], o["confidence"],
                                          o["right_view"], o["keep_aggr"]) if s["cn"] == 1 else False
    return q


# ---- the sequences one would write by hand ------------------------------------------------------------------------------------------
def sequence_same_frame_other_plan(name):
    """ONE frame shape on a living engine and its chained group while the plan under it changes: the engines of the group find
    their buffers sized for the frame (prepare_group's `sized` shortcut) and must still get what the new plan adds -- the raw
    records of the split winner-take-all and the maps of the two options at D = 128, the second to fifth volume, the int16
    row sums and the colour features at D = 64.  Runs behind the walk of engine `name`, on the same engine."""
    B = dict(entry="pipeline_batch_device", n=3, schedule=2, sweep_rows=3, keep_aggr=0, with_q=False)
    if name == "hh_d128":
        H, W = 40, 330
        return [step(H, W, 61, **B),                                                  # the split winner-take-all
                step(H, W, 62, **B, confidence=1, bind_conf=True),                     # ... off: a winner-take-all with the byte
                step(H, W, 63, **B, right_view=1, bind_right=True),
                step(H, W, 64, **dict(B, keep_aggr=1)),
                step(H, W, 65, **B),                                                  # ... and on again
                step(H, W, 66, **B, debug=256),                                        # the int16 cost pipeline: hsum
                step(H, W, 67, **B, cost=CENSUS, confidence=1, right_view=1, bind_conf=True, bind_right=True),
                step(H, W, 68, **B),
                step(H, W, 69, entry="compute_device", schedule=2, sweep_rows=3, keep_aggr=0, confidence=1, right_view=1),
                step(H, W, 70, entry="compute_device", schedule=2, sweep_rows=3, keep_aggr=0)]
    if name == "sgbm_d64_c3":
        H, W = 30, 250
        return [step(H, W, 71, **B),
                step(H, W, 72, **B, debug=2 | 2048),          # (the two winner-take-all bits at once: which of them a predicate asks)
                step(H, W, 73, **B, debug=256),
                step(H, W, 74, **B, cn=3),
                step(H, W, 75, **B, cost=CENSUS),
                step(H, W, 76, **dict(B, schedule=1, sweep_rows=0)),                    # five volumes
                step(H, W, 77, **dict(B, schedule=1, sweep_rows=0), debug=8192),        # three
                step(H, W, 78, **dict(B, schedule=1, sweep_rows=0), debug=8192 | 4096),  # two
                step(H, W, 79, **dict(B, schedule=1, sweep_rows=0), debug=8192 | 4096 | 65536),
                step(H, W, 80, **B, cn=3, confidence=1, bind_conf=True)]
    return []


def all_walks():
    """(name, parameters, steps)"""
    return [(ENGINES[i][0], ENGINES[i][1], make_walk(i)) for i in range(len(ENGINES))]
