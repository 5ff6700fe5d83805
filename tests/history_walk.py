"""Seeded walks of a long-lived engine, and what every step of them must compute (no GPU needed).

Shared by tests/history_child.py (which takes the walks on the GPU) and tests/test_history_walks.py (which regenerates
them with the oracle alone and checks how many steps leave the int16 regime).  A walk belongs to one parameter set --
parameters are fixed when an engine is created -- and draws, step after step, a shape, the options that are changed on
the living engine, an entry point and a stand-alone call in front of it.  Everything is a function of (engine index,
walk seed): a failing walk can be replayed as it was from the step list its failure message prints."""
from __future__ import annotations

import numpy as np

import bruteforce_color as BC
import bruteforce_hh4 as HH4
import parity_util as U
from oracle import oracle as O
from stereo_reconstruction_cv_amd import synth

# Poison bytes (csrc/sgm_debug.h: SGM_OPT_POISON).  The volumes are int16 and every path stage is a minimum: 0x80 is
# -32640 as a cost (wins every minimum), 0x7f is 32639 (next to SGM_MAX_COST: saturates sums); 0xff is -1 as a label and
# 0xffffffff as a winner-take-all key or minkey ("invalid": hides stale records, exposes counters and tickets); 0x01 is a
# small positive count in every word size (a component size, a run length, a ticket that is NOT zero).
POISON = (0x80, 0x7F, 0xFF, 0x01)

# SGM_OPT_DEBUG bits whose results stay bit-exact (csrc/sgm_debug.h; never 64)
DEBUG_BITS = (2, 4, 8, 16, 32, 128, 256, 512, 2048, 4096, 8192, 65536)

SP = dict(speckleWindowSize=30, speckleRange=2)
# (name, parameters, 3-channel-capable).  MODE_SGBM, MODE_HH and MODE_HH4, each at a small D, a lane-grouped D, 128 and
# 256 or 512.  Notebook penalties at block sizes 3 to 7 (inside the int16 regime for every input tried); the colour engine
# takes the plain ones, so that three channels' worth of cost stays inside it as well.
ENGINES = [
    ("sgbm_d32", U.params(32, 5, 0, 0, **SP), False),
    ("sgbm_d64_c3", U.params(64, 3, -5, 0, penalty="plain", **SP), True),
    ("sgbm_d128", U.params(128, 7, 0, 0, **SP), False),
    ("sgbm_d256", U.params(256, 5, 0, 0, speckleWindowSize=0, speckleRange=0), False),
    ("hh_d16", U.params(16, 7, 0, 1, **SP), False),
    ("hh_d48", U.params(48, 5, 3, 1, **SP), False),
    ("hh_d128", U.params(128, 5, 0, 1, **SP), False),
    ("hh_d512", U.params(512, 3, 0, 1, **SP), False),
    ("hh4_d32", U.params(32, 3, 0, 3, **SP), False),
    ("hh4_d64", U.params(64, 5, -8, 3, **SP), False),
    ("hh4_d128", U.params(128, 7, 0, 3, **SP), False),
    ("hh4_d256", U.params(256, 3, 0, 3, **SP), False),
]
STEPS = 20
WALK_SEED = 20240
ENTRIES = ("compute_host", "compute_device", "pipeline_device", "pipeline_batch_device", "compute_batch_host")
BETWEEN = ("none", "none", "trim", "median", "speckles", "to_float", "reproject", "reproject_missing", "mask", "compact", "rectify")
# elements of a cost volume per pair: keeps the taps small and the numpy restatements (MODE_HH4, colour) affordable
VOL_CAP, VOL_CAP_NUMPY = 6_000_000, 400_000


def width1(p, W: int) -> int:
    """columns that have a cost volume (W1 of the engine's geometry; <= 0: nothing matchable)"""
    return W + min(p["minDisparity"], 0) - max(p["minDisparity"] + p["numDisparities"], 0)


def make_walk(index: int, seed: int = WALK_SEED, steps: int = STEPS):
    """The steps of engine ENGINES[index]'s walk: a list of plain dicts."""
    name, p, colour = ENGINES[index]
    rng = np.random.default_rng(seed + 101 * index)
    D, minD, mode = p["numDisparities"], p["minDisparity"], p["mode"]
    edge = max(minD + D, 0) - min(minD, 0)      # the width at which W1 = 0
    out = []
    for k in range(steps):
        cn = 3 if colour and rng.integers(0, 2) else 1
        if k % 7 == 3:
            W = int(rng.integers(max(2, edge - 10), edge + 3))      # nothing or next to nothing matchable
        else:
            W = int(min(900, edge + rng.integers(1, 400)))
        H = int(rng.integers(1, 201))
        W1 = width1(p, W)
        cap = VOL_CAP_NUMPY if (mode == 3 or cn == 3) else VOL_CAP
        if W1 > 0:
            H = max(1, min(H, cap // (W1 * D)))
        entry = ENTRIES[int(rng.integers(0, len(ENTRIES)))]
        n = int(rng.integers(1, 6)) if "batch" in entry else 1
        if mode == 3 or cn == 3:
            n = min(n, 2)
        nbits = int(rng.integers(0, 3)) * int(rng.integers(0, 2))   # half of the steps: no debug bit; else one or two
        debug = 0
        for b in rng.choice(len(DEBUG_BITS), nbits, replace=False):
            debug |= DEBUG_BITS[int(b)]
        out.append(dict(
            k=k, H=H, W=W, cn=cn, noise=(k % 5 == 4), seed=int(rng.integers(0, 10 ** 6)), entry=entry, n=n,
            with_q=bool(rng.integers(0, 2)), pad=int(rng.integers(1, 40)),
            between=BETWEEN[int(rng.integers(0, len(BETWEEN)))], bseed=int(rng.integers(0, 10 ** 6)),
            opts=dict(schedule=int(rng.integers(0, 3)), sweep_rows=int(rng.choice([0, 0, 1, 2, 3, 5, 9])),
                      prepass_rows=int(rng.choice([0, 0, 3, 11, 64])), chain_wgs=int(rng.choice([0, 1, 2, 7])),
                      group_max=int(rng.choice([0, 1, 2, 3])), keep_aggr=int(rng.integers(0, 2)),
                      profile=int(rng.integers(0, 2)), debug=debug)))
    return out


def step(H, W, seed=1, entry="compute_host", n=1, cn=1, noise=False, with_q=True, pad=7, between="none", bseed=3, **opts):
    """A hand-written step (the deterministic sequences, the routes of the poison test)."""
    o = dict(schedule=1, sweep_rows=0, prepass_rows=0, chain_wgs=0, group_max=0, keep_aggr=1, profile=1, debug=0)
    assert set(opts) <= set(o), opts
    o.update(opts)
    return dict(k=-1, H=H, W=W, cn=cn, noise=noise, seed=seed, entry=entry, n=n, with_q=with_q, pad=pad, between=between,
                bseed=bseed, opts=o)


def pair(p, s, i=0):
    """Pair i of step s: a matchable synthetic pair, or plain noise (WTA ties, rejected pixels, speckles everywhere)."""
    H, W, cn, seed = s["H"], s["W"], s["cn"], s["seed"] + 7919 * i
    if s.get("special"):      # the hand-written inputs of sequence_out_of_regime_then_in
        if s["special"] == "overflow" and i == s["n"] - 1:
            return np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)
        soft = lambda a: (128 + (a.astype(int) - 128) // 8).astype(np.uint8)
        l, r, _ = synth.make_pair(H, W, p["numDisparities"], seed)
        return soft(l), soft(r)
    if s["noise"]:
        rng = np.random.default_rng(seed)
        shape = (H, W) if cn == 1 else (H, W, 3)
        return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
    if cn == 3:
        return BC.colour_pair(H, W, p["numDisparities"], seed, p["minDisparity"])
    l, r, _ = synth.make_pair(H, W, max(p["numDisparities"], 16), seed)
    return l, r


_cache: dict = {}


def expected(p, s, i=0):
    """What pair i of step s must give under parameters p: dict(disp, disp_raw, disp_median[, C, S], hr, ok).  hr is the
    headroom record (None for a colour pair, whose record the restatement does not form: only `ok` is known there);
    ok False: the input leaves the int16 regime and nothing but the engine's own verdict is compared.  Cached per
    (parameters, shape, channels, seed, noise)."""
    key = (tuple(sorted(p.items())), s["H"], s["W"], s["cn"], s["seed"], s["noise"], s.get("special"), i)
    if key in _cache:
        return _cache[key]
    l, r = pair(p, s, i)
    if width1(p, s["W"]) <= 0:
        # no volume at all: every pixel invalid whatever the path set and the channels
        m = lambda a: a if a.ndim == 2 else np.ascontiguousarray(a[..., 0])
        d, t = O.sgbm_compute(m(l), m(r), taps=True, **dict(p, mode=min(p["mode"], 1)))
        assert (d == (p["minDisparity"] - 1) * 16).all()
        e = dict(disp=d, disp_raw=t["disp_raw"], disp_median=t["disp_median"], ok=True,
                 hr=dict(ok=True, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"]))
    elif s["cn"] == 3:
        assert p["mode"] != 3, "no colour restatement of MODE_HH4 here"
        w = BC.sgbm_c3(l, r, **p)
        lim = int(w["C"].max()) + max(p["P2"], p["P1"] + 1)        # L_r <= C + P2
        e = dict(w, hr=None, ok=lim <= 32767)
    elif p["mode"] == 3:
        w = HH4.sgbm_hh4(l, r, **p)
        _, t = O.sgbm_compute(l, r, taps=True, **dict(p, mode=1))   # (the cost stage does not know the path set)
        assert np.array_equal(w["C"], t["C"])
        ok = t["max_cost_plus_p2"] <= 32767 and w["max_delta"] <= 32767
        e = dict(w, ok=ok, hr=dict(ok=ok, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=w["max_delta"]))
    else:
        d, t = O.sgbm_compute(l, r, taps=True, **p)
        ok = bool(t["headroom_ok"])
        e = dict(t, disp=d, ok=ok, hr=dict(ok=ok, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"]))
    _cache[key] = e
    return e


def step_ok(p, s):
    return all(expected(p, s, i)["ok"] for i in range(s["n"]))


def describe(name, p, steps, upto):
    """The prefix of a walk, one step per line, for a failure message."""
    lines = [f"engine {name} {p}"]
    for s in steps[:upto + 1]:
        lines.append(repr({k: v for k, v in s.items()}))
    return "\n".join(lines)


# ---- the two sequences one would write by hand ------------------------------------------------------------------------
def sequence_large_then_slivers():
    """A large noise frame under schedule 2, then a 1-row and a 1-column-of-W1 frame under schedules 1 and 0."""
    p = U.params(128, 5, 0, 1, **SP)
    steps = [step(180, 900, 41, noise=True, schedule=2, sweep_rows=5, chain_wgs=7)]
    for sched in (1, 0):
        steps += [step(1, 700, 42, schedule=sched), step(150, 129, 43, schedule=sched)]
    return "large_then_slivers", p, steps


OUT_OF_REGIME = dict(minDisparity=0, numDisparities=64, blockSize=11, P1=100, P2=24500, mode=1, disp12MaxDiff=1, preFilterCap=63,
                     uniquenessRatio=10, speckleWindowSize=0, speckleRange=0)


def sequence_out_of_regime_then_in():
    """An out-of-regime pair (constant 0 against constant 255 at blockSize = 11 with P2 = 24500: C + P2 > 32767), then an
    in-regime pair (a low-contrast one), through each entry point; the headroom record is checked after both."""
    steps = []
    for entry in ENTRIES:
        n = 3 if "batch" in entry else 1
        for sched in ((1, 2) if "batch" in entry else (1,)):
            steps += [dict(step(40, 300, 51, entry=entry, n=n, schedule=sched, group_max=2, with_q=False), special="overflow"),
                      dict(step(40, 300, 52, entry=entry, n=n, schedule=sched, group_max=2, with_q=False), special="soft")]
    # ... and across entry points: the overflowing pair of a chained batch runs on an internal engine of the group, and the
    # single compute behind it must not inherit that engine's record
    steps += [dict(step(40, 300, 53, entry="pipeline_batch_device", n=2, schedule=2, sweep_rows=4, with_q=False), special="overflow"),
              dict(step(40, 300, 54, entry="compute_host"), special="soft")]
    return "out_of_regime_then_in", dict(OUT_OF_REGIME), steps


def all_walks():
    """(name, parameters, steps, is_random_walk)"""
    out = [(ENGINES[i][0], ENGINES[i][1], make_walk(i), True) for i in range(len(ENGINES))]
    for seq in (sequence_large_then_slivers(), sequence_out_of_regime_then_in()):
        out.append(seq + (False,))
    return out
