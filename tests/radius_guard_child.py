"""Child process of tests/test_gpu_radius.py: its shape cases and a few of its extremes once under the engine's GUARDED allocation
mode (SGM_DEBUG_ALLOC=1, sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py).  The staged points, disparities and
colours, the table of cells, the sorted records, the per-point slot and rank words, the block counts and the five staged outputs
end where their mappings end, so a probe that leaves the table (k_radius_insert, k_radius_query), a run read past the sorted
records, a start written past the table (k_radius_starts) or an output row written past the kept points (k_radius_scatter) dies
here with a memory access fault, which ends THIS process, not the test session.  An engine per case, as in the other guard
children: every buffer then has exactly the case's size.  Prints one line `RADIUS_GUARD_OK <cases>` when everything ran and
matched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import radius_ref as RR
    from stereo_reconstruction_cv_amd import _lib
    from stereo_reconstruction_cv_amd.stereo import Engine

    def check(e, xyz, disp, col, r, nb, mc, o, want=None):
        if want is None:
            want = RR.cells(xyz, disp, col, r, nb, mc, o)
        p, c, keep, cnt, idx, noor = e.radius_outlier_host(xyz, disp, col, r, nb, mc, o, return_counts=True, return_index=True)
        assert p.shape[0] == want["n_kept"] and noor == want["n_out_of_range"], (p.shape, want["n_kept"], noor)
        assert np.array_equal(keep, want["keep"]) and np.array_equal(cnt, want["counts"]) and np.array_equal(idx, want["index"])
        assert np.array_equal(p.view(np.uint32), want["points"].view(np.uint32)) and (col is None or np.array_equal(c, want["colors"]))

    ncase = 0
    for i, case in enumerate(RR.SHAPE_CASES):                       # ten shapes
        xyz, disp, col = RR.case_input(i)
        check(Engine(dict(numDisparities=16)), xyz, disp, col, *case[3:], want=RR.case_want(i))
        ncase += 1
    xyz, disp, col = RR.layered_lists(48, 320, 704)
    far = np.array(xyz)
    far[5::7, 0] = 3.0e5
    own, _ = RR.lattice(16, 0.5)
    one = np.tile(np.array([[0.3, -0.2, 1.7]], np.float32), (4096, 1))
    T, S = _lib.SGM_DBG_RADIUS_TIGHT_TABLE, _lib.SGM_DBG_RADIUS_SOURCE_ORDER
    for debug, pts, d, c, r, nb, mc, o in (
            (0, one, None, None, 0.05, 8, 8, (0, 0, 0)),                  # one cell, stopping at max_count
            (0, one, None, None, 0.05, 8, RR.FULL, (0, 0, 0)),            # ... and counting it out
            (0, xyz, np.zeros_like(disp), col, 0.02, 1, 1, (0, 0, 0)),    # nothing valid
            (0, far, disp, None, 0.02, 8, 8, (0, 0, 0)),                  # out-of-range points among the others
            (0, xyz, None, col, 0.02, 5, 9, (0.013, -2.5, 100.0)),        # no disparities, an origin
            (T, own, None, None, 0.25, 1, 1, (0, 0, 0)),                  # load 1.0
            (T, xyz, disp, col, 0.02, 8, 8, (0, 0, 0)),
            (S, xyz, disp, col, 0.02, 8, RR.FULL, (0, 0, 0)),
            (T | S, xyz, disp, col, 0.01, 4, 6, (0, 0, 0))):
        e = Engine(dict(numDisparities=16))
        e.set_option(_lib.SGM_OPT_DEBUG, debug)
        check(e, pts, d, c, r, nb, mc, o)
        ncase += 1
    print(f"RADIUS_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
