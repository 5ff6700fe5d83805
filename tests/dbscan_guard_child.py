"""Child process of tests/test_gpu_dbscan.py: six of its shapes and a few of its extremes once under the engine's GUARDED
allocation mode (SGM_DEBUG_ALLOC=1, sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py).  The staged points and
disparities, the table of cells, the sorted records, the per-point slot words, the links, the nearest core points, the ranks, the
control words and the staged labels, core bytes and sizes end where their mappings end, so a probe that leaves the table or a run
read past the sorted records (k_dbscan_link), a link followed past the points (uf_find), a rank read for a point that is no root or
a size added past the clusters dies here with a memory access fault, which ends THIS process, not the test session.  An engine per
case, as in the other guard children: every buffer then has exactly the case's size.  Prints one line `DBSCAN_GUARD_OK <cases>` when
everything ran and matched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import dbscan_ref as DR
    from stereo_reconstruction_cv_amd import _lib
    from stereo_reconstruction_cv_amd.stereo import Engine

    def check(debug, xyz, disp, eps, k, o, want=None):
        e = Engine(dict(numDisparities=16))
        e.set_option(_lib.SGM_OPT_DEBUG, debug)
        if want is None:
            want = DR.cells(xyz, disp, eps, k, o)
        lab, core, sizes, st = e.cluster_dbscan_host(xyz, disp, eps, k, o, return_core=True, return_sizes=True)
        assert st.tolist() == want["stats"].tolist(), (st, want["stats"])
        assert np.array_equal(lab, want["labels"]) and np.array_equal(core, want["core"]) and np.array_equal(sizes, want["sizes"])

    ncase = 0
    GATHER, T = _lib.SGM_DBG_DBSCAN_GATHER_CORE, _lib.SGM_DBG_RADIUS_TIGHT_TABLE
    for i, debug in ((0, 0), (3, GATHER), (4, 0), (5, GATHER), (6, 0), (6, GATHER | T), (8, 0), (9, GATHER), (10, T)):   # six shapes
        xyz, disp = DR.case_input(i)
        check(debug, xyz, disp, *DR.SHAPE_CASES[i][3:], want=DR.case_want(i))
        ncase += 1
    xyz, disp = DR.layered_lists(24, 130, 724)
    far = np.array(xyz)
    far[5::7, 0] = 3.0e5
    one = np.tile(np.array([[0.3, -0.2, 1.7]], np.float32), (4096, 1))
    a, b = DR.two_chains(3000, 0.1)
    for debug, pts, d, eps, k, o in (
            (0, one, None, 0.05, 1, (0, 0, 0)),                      # one cell, one cluster: 4096 x 4095 / 2 pairs
            (GATHER, one, None, 0.05, 4096, (0, 0, 0)),              # all noise
            (0, xyz, np.zeros_like(disp), 0.05, 3, (0, 0, 0)),       # nothing valid
            (0, far, disp, 0.05, 3, (0, 0, 0)),                      # out-of-range points among the others
            (GATHER, far, disp, 0.05, 8, (0.013, -2.5, 100.0)),
            (T, np.concatenate([a, b]), None, 0.1, 1, (0, 0, 0))):   # two long chains, the table at the tight size
        check(debug, pts, d, eps, k, o)
        ncase += 1
    print(f"DBSCAN_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
