"""Child process of tests/test_gpu_right_view.py: four small rows with SGM_OPT_RIGHT_VIEW on under the engine's GUARDED
allocation mode (SGM_DEBUG_ALLOC=1, sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py).  Every volume ends
where its mapping ends, so a diagonal of k_right_wta that left its row at the LAST row -- or its volume anywhere -- would read
a guard page here, which ends THIS process, not the test session.  Rows: every diagonal truncated (W1 < D), a single
matched column (W1 = 1), a frame whose last row ends a tile exactly and one whose last tile is ragged, D = 1024.  Prints
one line `RIGHT_GUARD_OK <cases>` when everything ran and matched the reference."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import parity_util as U
    import right_view_ref as RR
    from oracle import oracle as O
    from stereo_reconstruction_cv_amd import _lib, synth
    from stereo_reconstruction_cv_amd.stereo import Engine

    ncase = 0
    for (H, W, D, minD, bs, mode, sched) in ((24, 90, 64, 0, 5, 0, 1), (8, 17, 16, 0, 3, 1, 1), (5, 256 + 32, 32, 0, 3, 0, 1),
                                             (7, 531, 48, 0, 5, 1, 1), (9, 1300, 1024, 0, 3, 1, 1)):
        l, r, _ = synth.make_pair(H, W, D, 9950 + D + mode)
        p = U.params(D, bs, minD, mode, speckleWindowSize=30, speckleRange=2)
        want, t = O.sgbm_compute(l, r, taps=True, **p)
        assert t["headroom_ok"], (H, W, D, mode)
        minX1 = W - t["S"].shape[1] + min(minD, 0)
        raw, fin = RR.right_view(t["S"], W, minX1, p)
        eng = Engine(p)
        eng.set_option(_lib.SGM_OPT_SCHEDULE, sched)
        eng.set_option(_lib.SGM_OPT_RIGHT_VIEW, 1)
        for rep in range(2):
            got = eng.compute_host(l, r)
            assert np.array_equal(got, want), (H, W, D, mode, rep)
            assert np.array_equal(eng.tap(_lib.SGM_TAP_RIGHT_RAW, H, W), raw), (H, W, D, mode, rep)
            assert np.array_equal(eng.tap(_lib.SGM_TAP_RIGHT, H, W), fin), (H, W, D, mode, rep)
        ncase += 1
    print(f"RIGHT_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
