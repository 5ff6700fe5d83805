"""An engine's results must not depend on its history -- over everything that was added since tests/test_gpu_history.py was
written (needs an MI355X).

Eight long-lived engines, one child process each (tests/feature_walk_child.py), take the seeded walks of
tests/feature_walk.py: numDisparities up to 1024, the cost function, the confidence and the right-view option flipped on the
living engine, their maps through the taps or through the bind entries, and in front of every compute one of the stand-alone
calls that share buffers with it (the edge-aware filter, the left-right confidence, the voxel grid, the two outlier filters,
the mesh, the normals) -- once plain and once with every buffer poisoned in front of every call.  Everything is compared bit
for bit with the references the feature tests use.  tests/test_feature_walks.py holds, without a GPU, the conditions under
which a walk that passes means something.  The point-cloud calls added later are walked in tests/cloud_walk.py
(tests/test_gpu_cloud_walk.py).

A child that ends by a signal, by an abort or at its time limit has met a fault or a hang: nothing more is started on the
card after it.  That test fails, and the walks behind it skip with its reason."""
import os
import re
import subprocess
import sys

import pytest

import feature_walk as FW
from feature_walk_child import NEW_STAGES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Seconds per child, interpreter and torch start-up included, measured once on an MI355X (profiles/feature_walks/times.json):
# sgbm_d32 2.97, sgbm_d64_c3 3.10, sgbm_d160 3.08, hh_d128 4.06, hh_d256 3.24, hh4_d48_c3 2.71, hh4_d528 3.53, hh_d1024 3.47.
# The limit is five times the slowest (20.3 s), rounded up to the next 10 s (30 s) and at least 60 s: the factor covers a cold
# code-object load and a busy 16-CPU allotment, it is not there for slow kernels.
CHILD_TIMEOUT = 60

_seen: dict = {}         # engine name -> the stage names its child saw
_stopped: list = []      # why no further child is started


@pytest.mark.parametrize("name", FW.NAMES)
def test_walk_of_one_engine_plain_and_poisoned(name):
    """16 steps, twice: every compute and every call in front of it equal to the references, bit for bit"""
    if _stopped:
        pytest.skip(f"no further child on this card: {_stopped[0]}")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "feature_walk_child.py"), name], capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as x:
        _stopped.append(f"the walk of {name} did not end within {CHILD_TIMEOUT} s")
        pytest.fail(_stopped[0] + "\n" + str(x.stdout or "")[-3000:])
    tail = (r.stdout + r.stderr)[-8000:]
    if r.returncode < 0 or r.returncode in (134, 137, 139):
        _stopped.append(f"the walk of {name} ended with status {r.returncode}")
        pytest.fail(_stopped[0] + "\n" + tail)
    assert r.returncode == 0, tail
    m = re.search(r"^FEATURE_WALK_OK (\d+)((?: \w+)*)$", r.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 2 * FW.STEPS, tail
    _seen[name] = set(m.group(2).split())


def test_the_walks_together_ran_every_stage_added_since_the_history_walks():
    if _stopped:
        pytest.skip(f"no further child on this card: {_stopped[0]}")
    assert set(_seen) == set(FW.NAMES), sorted(set(FW.NAMES) - set(_seen))        # (run the whole module)
    seen = set().union(*_seen.values())
    missing = [nm for nm in NEW_STAGES if nm not in seen]
    assert not missing, f"no walk ran these stages: {missing}"
