"""An engine's results must not depend on its history -- over the point-cloud calls that were added since
tests/test_gpu_feature_walk.py was written (needs an MI355X).

Four long-lived engines, one child process each (tests/cloud_walk_child.py), take the seeded walks of tests/cloud_walk.py:
sgm_covariance_normals, sgm_cluster_dbscan, sgm_segment_plane, sgm_plane_inliers, sgm_register_icp, sgm_evaluate_registration,
sgm_transform_points, sgm_tsdf_integrate and sgm_tsdf_extract_points among the older calls that share the cell grid, the keep
byte, the counts, the scan and the staging buffers with them, a trim, a refusal and a compute -- clouds replayed under another
call, empty clouds behind full grids, one volume alive through the walk -- once plain and once with every buffer poisoned in
front of every call.  Everything is compared bit for bit with the references the calls' own tests use.
tests/test_cloud_walks.py holds, without a GPU, the conditions under which a walk that passes means something.

A child that ends by a signal, by an abort or at its time limit has met a fault or a hang: nothing more is started on the
card after it.  That test fails, and the walks behind it skip with its reason."""
import os
import re
import subprocess
import sys

import pytest

import cloud_walk as CW
from stereo_reconstruction_cv_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Seconds per child, interpreter and torch start-up included, measured once on an MI355X (profiles/cloud_walks/times.json):
# sgbm_d32 3.03, sgbm_d64_c3 2.75, hh_d128 3.02, hh4_d48_c3 2.78.
# The limit is five times the slowest (15.2 s), rounded up to the next 10 s (20 s) and at least 60 s: the factor covers a cold
# code-object load and a busy 16-CPU allotment, it is not there for slow kernels.
CHILD_TIMEOUT = 60
NEW_STAGES = _lib.COVARIANCE_STAGES + _lib.DBSCAN_STAGES + _lib.PLANE_STAGES + _lib.ICP_STAGES + _lib.TSDF_STAGES

_seen: dict = {}         # engine name -> the stage names its child saw
_stopped: list = []      # why no further child is started


@pytest.mark.parametrize("name", CW.NAMES)
def test_walk_of_one_engine_plain_and_poisoned(name):
    """24 steps, twice: every call equal to its reference, bit for bit"""
    if _stopped:
        pytest.skip(f"no further child on this card: {_stopped[0]}")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cloud_walk_child.py"), name], capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as x:
        _stopped.append(f"the walk of {name} did not end within {CHILD_TIMEOUT} s")
        pytest.fail(_stopped[0] + "\n" + str(x.stdout or "")[-3000:])
    tail = (r.stdout + r.stderr)[-8000:]
    if r.returncode < 0 or r.returncode in (134, 137, 139):
        _stopped.append(f"the walk of {name} ended with status {r.returncode}")
        pytest.fail(_stopped[0] + "\n" + tail)
    assert r.returncode == 0, tail
    m = re.search(r"^CLOUD_WALK_OK (\d+)((?: \w+)*)$", r.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 2 * CW.STEPS, tail
    _seen[name] = set(m.group(2).split())


def test_the_walks_together_ran_every_stage_of_the_calls_added_since_the_feature_walks():
    """(cov_solve needs SGM_DBG_COV_SEPARATE_SOLVE on a profiled step, plane_moments and plane_solve refine = 1 on one)"""
    if _stopped:
        pytest.skip(f"no further child on this card: {_stopped[0]}")
    assert set(_seen) == set(CW.NAMES), sorted(set(CW.NAMES) - set(_seen))        # (run the whole module)
    seen = set().union(*_seen.values())
    missing = [nm for nm in NEW_STAGES if nm not in seen]
    assert not missing, f"no walk ran these stages: {missing}"
