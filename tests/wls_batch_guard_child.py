"""Child process of tests/test_gpu_wls_batch.py: batches of the edge-aware disparity filter under the engine's GUARDED allocation
mode (SGM_DEBUG_ALLOC=1, sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py), through the host entry.  The three
float planes [C][H][W] and the staged maps, guides and confidence maps of a chunk end where their mappings end, so the LAST map
of a chunk is the one whose neighbour reads (guide[i + 1] in k_wls_rows, guide[i + W] in k_wls_cols) or tile rows past its
last pixel would die here with a memory access fault, which ends THIS process, not the test session; a map in the middle that
strays into its neighbour's plane shows as a wrong result instead.  Ragged tails in both directions, degenerate lines, a batch
cut into chunks.  An engine per case (the regrow finding): every buffer then has exactly the case's size.
Prints one line `WLS_BATCH_GUARD_OK <cases>` when everything ran and matched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402

# (N, H, W, cn, conf, lambda, sigma, invalid, SGM_OPT_GROUP_MAX)
CASES = [(4, 65, 129, 1, True, 8000.0, 1.5, -16, 0), (3, 130, 67, 3, False, 100.0, 10.0, -160, 0), (2, 200, 33, 1, True, 8000.0, 0.5, -16, 0),
         (3, 97, 260, 3, True, 1e6, 1.5, -160, 2), (2, 1, 7, 3, False, 8000.0, 1.5, -16, 0), (3, 7, 1, 1, True, 100.0, 10.0, -160, 0)]


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import wls_ref as WR
    from stereo_reconstruction_cv_amd import _lib
    from stereo_reconstruction_cv_amd.stereo import Engine

    ncase = 0
    for (N, H, W, cn, with_conf, lam, sigma, invalid, group_max) in CASES:
        eng = Engine(dict(numDisparities=16))
        eng.set_option(_lib.SGM_OPT_GROUP_MAX, group_max)
        ins = [WR.random_input(H, W, cn, 500 + 10 * ncase + i, invalid, with_conf=with_conf) for i in range(N)]
        lut = WR.weights(sigma)
        out, outf = eng.wls_filter_batch_host(np.stack([s["disp"] for s in ins]), np.stack([s["guide"] for s in ins]),
                                              np.stack([s["conf"] for s in ins]) if with_conf else None, invalid, lam, lut,
                                              return_float=True)
        for i, s in enumerate(ins):
            want = WR.wls_filter(s["disp"], s["guide"], s["conf"], invalid, lam, lut)
            assert np.array_equal(out[i], want["out"]), (N, H, W, cn, i)
            assert np.array_equal(outf[i].view(np.uint32), want["out_f32"].view(np.uint32)), (N, H, W, cn, i)
        ncase += 1
    print(f"WLS_BATCH_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
