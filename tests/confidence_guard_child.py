"""Child process of tests/test_gpu_confidence.py: seven small rows with SGM_OPT_CONFIDENCE on under the engine's GUARDED
allocation mode (SGM_DEBUG_ALLOC=1, sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py).  The two uint8 maps
end where their mapping ends, so a byte written past the last pixel -- by k_wta_conf_t's store or by the four-pixel form of
k_conf_final on a frame whose pixel count is not a multiple of four -- dies here with a memory access fault, which ends THIS
process, not the test session.  Prints one line `CONF_GUARD_OK <cases>` when everything ran and matched the reference."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import confidence_ref as CR
    import parity_util as U
    from oracle import oracle as O
    from oracle import volume_oracle as V
    from stereo_reconstruction_cv_amd import _lib, synth
    from stereo_reconstruction_cv_amd.stereo import Engine

    ncase = 0
    # odd pixel counts (H * W % 4 != 0), every number of volumes (5, 2, 1, 4), the diverted routes (D = 256 MODE_SGBM,
    # schedule 0, D = 1024 with its 131 KB of LDS), the chained schedule, both signs of the uniqueness weight
    for (H, W, D, minD, bs, mode, uniq, sched) in ((13, 101, 16, 0, 5, 0, 10, 1), (11, 203, 128, -3, 5, 0, 100, 1),
                                                   (9, 391, 256, 0, 5, 0, 10, 1), (21, 181, 64, 2, 3, 1, 10, 0),
                                                   (7, 1024 + 131, 1024, 0, 3, 1, 10, 1), (15, 163, 48, 0, 5, 3, 10, 1),
                                                   (31, 333, 128, 0, 5, 1, 150, 2)):
        l, r, _ = synth.make_pair(H, W, D, 9900 + D + mode)
        p = U.params(D, bs, minD, mode, uniquenessRatio=uniq, speckleWindowSize=30, speckleRange=2)
        want, t = (V if mode == 3 else O).sgbm_compute(l, r, taps=True, **p)
        assert t["headroom_ok"], (H, W, D, mode)
        minX1 = W - t["S"].shape[1] + min(minD, 0)
        raw = CR.conf_raw(t["S"], W, minX1)
        eng = Engine(p)
        eng.set_option(_lib.SGM_OPT_SCHEDULE, sched)
        eng.set_option(_lib.SGM_OPT_CONFIDENCE, 1)
        for rep in range(2):
            got = eng.compute_host(l, r)
            assert np.array_equal(got, want), (H, W, D, mode, rep)
            assert np.array_equal(eng.tap(_lib.SGM_TAP_CONF_RAW, H, W), raw), (H, W, D, mode, rep)
            assert np.array_equal(eng.tap(_lib.SGM_TAP_CONF, H, W), CR.conf_final(raw, want, minD)), (H, W, D, mode, rep)
        ncase += 1
    print(f"CONF_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
