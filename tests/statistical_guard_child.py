"""Child process of tests/test_gpu_statistical.py: its shape cases and a few of its extremes once under the engine's GUARDED
allocation mode (SGM_DEBUG_ALLOC=1, sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py).  The staged points,
disparities and colours, the table of cells, the sorted records, the per-point slot and q words, the 64-bit sums, the block counts
and the five staged outputs end where their mappings end, so a probe that leaves the table or a run read past the sorted records
(k_stat_query), a q or a mean written past the points, or an output row written past the kept points dies here with a memory
access fault, which ends THIS process, not the test session.  An engine per case, as in the other guard children: every buffer
then has exactly the case's size.  Prints one line `STATISTICAL_GUARD_OK <cases>` when everything ran and matched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import statistical_ref as SR
    from stereo_reconstruction_cv_amd import _lib
    from stereo_reconstruction_cv_amd.stereo import Engine

    def check(e, xyz, disp, col, k, ratio, r, o, want=None):
        if want is None:
            want = SR.cells(xyz, disp, col, k, ratio, r, o)
        p, c, keep, mean, idx, st = e.statistical_outlier_host(xyz, disp, col, k, ratio, r, o, return_distances=True, return_index=True)
        assert p.shape[0] == want["n_kept"] and st.tolist() == want["stats"].tolist(), (p.shape, want["n_kept"], st, want["stats"])
        assert np.array_equal(keep, want["keep"]) and np.array_equal(mean.view(np.uint32), want["mean"].view(np.uint32))
        assert np.array_equal(idx, want["index"])
        assert np.array_equal(p.view(np.uint32), want["points"].view(np.uint32)) and (col is None or np.array_equal(c, want["colors"]))

    ncase = 0
    for i, case in enumerate(SR.SHAPE_CASES):                       # ten shapes
        xyz, disp, col = SR.case_input(i)
        check(Engine(dict(numDisparities=16)), xyz, disp, col, *case[3:], want=SR.case_want(i))
        ncase += 1
    xyz, disp, col = SR.layered_lists(48, 320, 704)
    small = SR.layered_lists(24, 130, 724)
    far = np.array(xyz)
    far[5::7, 0] = 3.0e5
    own, _ = SR.lattice(16, 0.5)
    one = np.tile(np.array([[0.3, -0.2, 1.7]], np.float32), (4096, 1))
    T = _lib.SGM_DBG_RADIUS_TIGHT_TABLE
    for debug, pts, d, c, k, ratio, r, o in (
            (0, one, None, None, 64, 1.0, 0.05, (0, 0, 0)),                   # one cell, every list full of zeros
            (0, xyz, np.zeros_like(disp), col, 1, 1.0, 0.02, (0, 0, 0)),      # nothing valid
            (0, far, disp, None, 8, 1.0, 0.02, (0, 0, 0)),                    # out-of-range points among the others
            (0, xyz, None, col, 5, 0.5, 0.02, (0.013, -2.5, 100.0)),          # no disparities, an origin
            (0, *small, 9, 1.0, 0.05, (0, 0, 0)),                             # one instance of k_stat_query per capacity
            (0, *small, 17, 1.0, 0.05, (0, 0, 0)),
            (0, *small, 33, 1.0, 0.05, (0, 0, 0)),
            (0, *small, 64, 1.0, 0.1, (0, 0, 0)),
            (T, own, None, None, 6, 1.0, 0.5, (0, 0, 0)),                     # load 1.0
            (T, xyz, disp, col, 8, 1.0, 0.02, (0, 0, 0))):
        e = Engine(dict(numDisparities=16))
        e.set_option(_lib.SGM_OPT_DEBUG, debug)
        check(e, pts, d, c, k, ratio, r, o)
        ncase += 1
    print(f"STATISTICAL_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
