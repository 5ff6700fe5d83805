"""Child process of tests/test_gpu_census.py: seven small rows with SGM_OPT_COST = SGM_COST_CENSUS under the engine's GUARDED
allocation mode (SGM_DEBUG_ALLOC=1, sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py).  The descriptor
buffers (8 bytes per pixel and image) and the byte volume end where their mappings end, so a descriptor read past the last
pixel of an odd-sized frame by k_pix_census*, or a byte stored past the volume, dies here with a memory access fault, which
ends THIS process, not the test session.  Prints one line `CENSUS_GUARD_OK <cases>` when everything ran and matched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import census_ref as CE
    import parity_util as U
    from stereo_reconstruction_cv_amd import _lib, synth
    from stereo_reconstruction_cv_amd.stereo import Engine

    ncase = 0
    # odd pixel counts; the thread-per-pixel form (D = 16), the wave form at NP = 1, 2, 4 and 8 (D = 1024); k_box_u8 and
    # the int16 route (blockSize 1 behind the wave form and behind the
    # thread-per-pixel form, debug 256, D > 512); a frame shorter than the census window
    for (H, W, D, minD, bs, mode, sched, debug) in ((13, 101, 16, 0, 5, 0, 1, 0), (11, 203, 128, -3, 5, 1, 1, 0),
                                                    (9, 391, 256, 0, 1, 0, 1, 0), (5, 181, 64, 2, 3, 1, 0, 256),
                                                    (7, 1024 + 131, 1024, 0, 3, 1, 1, 0), (15, 463, 272, 0, 5, 3, 2, 0),
                                                    (9, 77, 32, 0, 1, 0, 1, 0)):
        l, r, _ = synth.make_pair(H, W, D, 9900 + D + mode)
        p = U.params(D, bs, minD, mode, speckleWindowSize=30, speckleRange=2)
        t = CE.census_sgbm(l, r, **p)
        assert t["headroom"]["ok"], (H, W, D, mode)
        eng = Engine(p)
        eng.set_option(_lib.SGM_OPT_COST, _lib.SGM_COST_CENSUS)
        eng.set_option(_lib.SGM_OPT_SCHEDULE, sched)
        if debug:
            eng.set_option(_lib.SGM_OPT_DEBUG, debug)
        for rep in range(2):
            got = eng.compute_host(l, r)
            assert np.array_equal(eng.tap(_lib.SGM_TAP_COST, H, W), t["C"]), (H, W, D, mode, rep)
            assert np.array_equal(got, t["disp"]), (H, W, D, mode, rep)
            assert eng.headroom() == t["headroom"], (H, W, D, mode, rep)
        ncase += 1
    print(f"CENSUS_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
