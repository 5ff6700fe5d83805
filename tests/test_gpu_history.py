"""An engine's results must not depend on its history (needs an MI355X).

Almost every other GPU test looks at an engine that was just created: its buffers come straight from the allocator, and
whatever such memory holds, zero is the friendliest content there is for this code (a zero component size, a zero cost,
a zero ticket).  The engine is built for the opposite -- device memory lives in it and is reused between calls, some
forty buffers carry one call's bytes into the next, and which of them a call needs depends on a plan that depends on
shape, options and debug bits.  So here

  * every route make_plan can take and every entry point that owns buffers starts from buffers filled with a hostile
    byte (SGM_OPT_POISON, csrc/sgm_debug.h) -- with the condition that the routes' stage names cover everything
    run_compute can emit (tests/history_child.py: STAGES);
  * long-lived engines, one per parameter set, take seeded walks through shapes, options and entry points
    (tests/history_walk.py), once plain and once poisoned between the steps, and two hand-written sequences beside them;
  * the cv2-style setters change a StereoSGBM between computes, and more parameter sets than the engine cache holds are
    cycled through it.

Everything is compared bit-exactly with the oracle.  The poisoned parts run in a child process under a time limit, as
tests/test_gpu_guard.py does: a read-before-write of a buffer that holds indices could turn poison into a wild address,
and that must end the child, not the session (DESIGN.md 4.9 records why no such read is expected)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import parity_util as U
from oracle import oracle as O
from stereo_reconstruction_cv_amd import synth
from stereo_reconstruction_cv_amd import stereo as cv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(part, at_least, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "history_child.py"), part], capture_output=True, text=True,
                       timeout=timeout)
    tail = (r.stdout + r.stderr)[-6000:]
    assert r.returncode == 0, tail
    m = re.search(r"HISTORY_OK (\d+)", r.stdout)
    assert m and int(m.group(1)) >= at_least, tail


def test_every_route_from_poisoned_buffers():
    """87 routes x 4 poison bytes; the union of their stage names contains every stage the engine can emit."""
    _child("routes", 4 * 87, 600)


def test_walks_of_long_lived_engines_plain_and_poisoned():
    """12 seeded walks of 20 steps and the two hand-written sequences, each once plain and once with every buffer
    poisoned in front of every stand-alone call and every compute."""
    _child("walks", 2 * (12 * 20 + 5 + 16), 900)


def _want(l, r, p):
    d, t = O.sgbm_compute(l, r, taps=True, **p)
    assert t["headroom_ok"], p
    return d


def test_setters_between_computes_on_one_matcher():
    """cv2-style setters on a living StereoSGBM: every compute answers for the parameters then in force."""
    H, W = 60, 420
    l, r, _ = synth.make_pair(H, W, 128, 901)
    p = U.params(64, 5, 0, 0)
    m = cv.StereoSGBM_create(**p)
    assert np.array_equal(m.compute(l, r), _want(l, r, p))
    for setter, field, value in (("setNumDisparities", "numDisparities", 128), ("setBlockSize", "blockSize", 7),
                                 ("setMode", "mode", 1), ("setMinDisparity", "minDisparity", -6), ("setP1", "P1", 200),
                                 ("setP2", "P2", 1500), ("setSpeckleWindowSize", "speckleWindowSize", 0),
                                 ("setNumDisparities", "numDisparities", 16), ("setMode", "mode", 0),
                                 ("setSpeckleWindowSize", "speckleWindowSize", 60), ("setNumDisparities", "numDisparities", 64),
                                 ("setBlockSize", "blockSize", 5), ("setMinDisparity", "minDisparity", 0)):
        getattr(m, setter)(value)
        p[field] = value
        assert getattr(m, "g" + setter[1:])() == value
        got = m.compute(l, r)
        want = _want(l, r, p)
        assert np.array_equal(got, want), (setter, value, int((got != want).sum()))


def test_engine_cache_eviction_and_recreation():
    """Seven parameter sets cycled twice through get_engine (the cache holds four): engines are evicted and created
    again, numpy and device-tensor inputs alternate, every result is the oracle's."""
    import torch
    cv.clear_engine_cache()
    sets = [U.params(D, bs, minD, mode) for D, bs, minD, mode in ((16, 3, 0, 0), (64, 5, 0, 1), (128, 7, 0, 0), (256, 5, 0, 1),
                                                                   (48, 3, 4, 0), (128, 5, -8, 1), (32, 7, 0, 1))]
    assert len(sets) > cv._CACHE_MAX
    shapes = [(40, 330), (75, 520), (23, 700), (120, 400)]
    n = 0
    for cycle in range(2):
        for i, p in enumerate(sets):
            H, W = shapes[(i + cycle) % len(shapes)]
            l, r, _ = synth.make_pair(H, W, max(p["numDisparities"], 16), 950 + 10 * cycle + i)
            m = cv.StereoSGBM_create(**p)
            if (i + cycle) % 2:
                got = m.compute(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()).cpu().numpy()
            else:
                got = m.compute(l, r)
            want = _want(l, r, p)
            assert np.array_equal(got, want), (cycle, i, int((got != want).sum()))
            assert len(cv._engine_cache) <= cv._CACHE_MAX
            n += 1
    assert n == 14
    cv.clear_engine_cache()
