"""Child process of tests/test_gpu_covariance.py: six of its shapes and a few of its extremes once under the engine's GUARDED
allocation mode (SGM_DEBUG_ALLOC=1, sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py).  The staged points and
disparities, the table of cells, the sorted records, the per-point slot words, the control words, the staged moments and the three
staged outputs end where their mappings end, so a probe that leaves the table or a run read past the sorted records (k_cov_query),
ten words staged past the points in range, or a normal, curvature or count written past the points dies here with a memory access
fault, which ends THIS process, not the test session.  An engine per case, as in the other guard children: every buffer then has
exactly the case's size.  Prints one line `COVARIANCE_GUARD_OK <cases>` when everything ran and matched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import covariance_ref as CR
    from stereo_reconstruction_cv_amd import _lib
    from stereo_reconstruction_cv_amd.stereo import Engine

    def check(debug, xyz, disp, r, k, o, w, orient, want=None):
        e = Engine(dict(numDisparities=16))
        e.set_option(_lib.SGM_OPT_DEBUG, debug)
        if want is None:
            want = CR.cells(xyz, disp, r, k, o, w, bool(orient))
        nrm, curv, cnt, st = e.covariance_normals_host(xyz, disp, r, k, o, w, bool(orient), return_curvature=True, return_counts=True)
        assert st.tolist() == want["stats"].tolist(), (st, want["stats"])
        assert np.array_equal(nrm.view(np.uint32), want["normals"].view(np.uint32)) and np.array_equal(cnt, want["counts"])
        assert np.array_equal(curv.view(np.uint32), want["curvature"].view(np.uint32))

    ncase = 0
    SEP, SEL, T = _lib.SGM_DBG_COV_SEPARATE_SOLVE, _lib.SGM_DBG_COV_SELECT_ACCUM, _lib.SGM_DBG_RADIUS_TIGHT_TABLE
    for i, debug in ((0, 0), (3, SEP), (4, 0), (5, SEP), (6, SEL), (7, SEP | SEL), (8, 0), (8, SEP), (9, 0), (9, SEP | T)):   # six shapes
        xyz, disp = CR.case_input(i)
        check(debug, xyz, disp, *CR.SHAPE_CASES[i][3:], want=CR.case_want(i))
        ncase += 1
    xyz, disp = CR.layered_lists(24, 130, 724)[:2]
    far = np.array(xyz)
    far[5::7, 0] = 3.0e5
    one = np.tile(np.array([[0.3, -0.2, 1.7]], np.float32), (4096, 1))
    own = CR.plane_lattice(32, 32)
    for debug, pts, d, r, k, o in (
            (0, one, None, 0.05, 64, (0, 0, 0)),                     # one cell, every point degenerate
            (SEP, one, None, 0.05, 64, (0, 0, 0)),
            (0, xyz, np.zeros_like(disp), 0.05, 3, (0, 0, 0)),       # nothing valid
            (0, far, disp, 0.05, 3, (0, 0, 0)),                      # out-of-range points among the others
            (SEP, far, disp, 0.05, 3, (0.013, -2.5, 100.0)),
            (T, own, None, 0.5, 5, (0, 0, 0))):                      # 1024 points in a table of 1024 slots
        check(debug, pts, d, r, k, o, (0.5, 0.25, -1.0), 1)
        ncase += 1
    print(f"COVARIANCE_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
