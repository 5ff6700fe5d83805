"""Child process of tests/test_gpu_lrc.py: the shape list of the left-right consistency confidence once under the engine's
GUARDED allocation mode (SGM_DEBUG_ALLOC=1, sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py).  The staged maps,
the base, the two results and the factor planes end where their mappings end, so a halo pixel fetched past the last row of a map
(k_lrc_factor), a factor stored past a plane, or a gather at a match column outside the row (k_lrc_match) dies here with a
memory access fault, which ends THIS process, not the test session.  An engine per case, as in the other guard children: every
buffer then has exactly the case's size.  Prints one line `LRC_GUARD_OK <cases>` when everything ran and matched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import lrc_ref as LR
    from stereo_reconstruction_cv_amd.stereo import Engine

    ncase = 0
    for i, (H, W, r, T, V, invalid, levels) in enumerate(LR.SHAPE_CASES):
        eng = Engine(dict(numDisparities=16))
        s = LR.case_input(i)
        wl, wr = LR.case_want(i)
        cl, cr = eng.lrc_confidence_host(s["dl"], s["dr"], s["base"], invalid, T, r, V, True, True)
        assert np.array_equal(cl, wl) and np.array_equal(cr, wr), (H, W, r)
        ncase += 1
    print(f"LRC_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
