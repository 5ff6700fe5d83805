"""Child process of tests/test_gpu_wls.py: the shape list of the edge-aware disparity filter once under the engine's GUARDED
allocation mode (SGM_DEBUG_ALLOC=1, sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py).  The three float planes
and the staged map, guide and confidence end where their mappings end, so a neighbour read past the last pixel of a line
(guide[i + 1] in k_wls_rows, guide[i + W] in k_wls_cols) or a tile row stored past a plane dies here with a memory access fault,
which ends THIS process, not the test session.  A single map is a chunk of one of the same kernels the batch entries run
(csrc/kernels_wls.h), in the shape the library picks for such a chunk.  An engine per case, as in the other guard children: every buffer then has exactly
the case's size.  Prints one line `WLS_GUARD_OK <cases>` when everything ran and matched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import wls_ref as WR
    from stereo_reconstruction_cv_amd.stereo import Engine

    ncase = 0
    for (H, W, cn, with_conf, lam, sigma, invalid) in WR.SHAPE_CASES:
        eng = Engine(dict(numDisparities=16))
        s = WR.random_input(H, W, cn, 300 + ncase, invalid, with_conf=with_conf)
        lut = WR.weights(sigma)
        want = WR.wls_filter(s["disp"], s["guide"], s["conf"], invalid, lam, lut)
        out, outf = eng.wls_filter_host(s["disp"], s["guide"], s["conf"], invalid, lam, lut, return_float=True)
        assert np.array_equal(out, want["out"]), (H, W, cn)
        assert np.array_equal(outf.view(np.uint32), want["out_f32"].view(np.uint32)), (H, W, cn)
        ncase += 1
    print(f"WLS_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
