"""Child process of tests/test_gpu_wide_disparity.py: six small rows with numDisparities > 512 under the engine's GUARDED
allocation mode (SGM_DEBUG_ALLOC=1, sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py).  A lane of the
NP = 8 kernels moves 32 bytes per access -- two 128-bit loads, four 64-bit stores -- so an access that starts inside a row
and runs past the end of the volume dies here with a memory access fault, which ends THIS process, not the test session.
Prints one line `WIDE_GUARD_OK <cases>` when everything ran and matched the oracles."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import bruteforce_color as BC
    import parity_util as U
    from oracle import volume_oracle as V
    from stereo_reconstruction_cv_amd import _lib, synth
    from stereo_reconstruction_cv_amd.stereo import Engine

    ncase = 0
    # full (D = 1024) and partial waves, both modes, the last chunk of a row 1, 3 and 127 columns wide (W1 % 128), the
    # generic vertical sum (window 13), the one-kernel-per-direction and the chained schedule option
    for (H, W, D, bs, mode, sched) in ((9, 1024 + 129, 1024, 5, 1, 1), (11, 1024 + 131, 1024, 3, 0, 2), (9, 528 + 255, 528, 5, 1, 0),
                                       (10, 1008 + 140, 1008, 13, 0, 1), (13, 640 + 133, 640, 7, 1, 2)):
        l, r, _ = synth.make_pair(H, W, D, 9700 + D + bs)
        p = U.params(D, bs, 0, mode, speckleWindowSize=30, speckleRange=2)
        rep, t, h = U.compare_stages(l, r, p, schedule=sched)
        assert t["headroom_ok"], (H, W, D, bs, mode)
        bad = [U.describe_mismatch(k, h[k], t[k]) for k, n in rep.items() if n]
        assert not bad, f"{(H, W, D, bs, mode, sched)}: " + "\n".join(bad)
        ncase += 1
    # one colour pair (k_hsum<8, ., 3>)
    H, W, D = 9, 1024 + 130, 1024
    L3, R3 = BC.colour_pair(H, W, D, seed=9800)
    p = U.params(D, 3, 0, 1, penalty="plain", speckleWindowSize=12, speckleRange=2)
    want, t = V.sgbm_compute(L3, R3, taps=True, **p)
    assert t["headroom_ok"]
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_KEEP_AGGR, 1)
    got = eng.compute_host(L3, R3)
    assert np.array_equal(eng.tap(_lib.SGM_TAP_COST, H, W), t["C"]) and np.array_equal(eng.tap(_lib.SGM_TAP_AGGR, H, W), t["S"])
    assert np.array_equal(got, want)
    assert eng.headroom() == dict(ok=True, max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"])
    ncase += 1
    print(f"WIDE_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
