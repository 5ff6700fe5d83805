"""Child process of tests/test_gpu_tsdf.py: some of its cases once under the engine's GUARDED allocation mode (SGM_DEBUG_ALLOC=1,
sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py).  The staged planes, the staged frame, the blocks' counts and
offsets and the staged rows end where their mappings end, so a voxel past V, a pixel past the frame (k_tsdf_integrate), a neighbour
past a face of the volume (k_tsdf_count, k_tsdf_emit), an offset past the blocks or a row past the capacity dies here with a memory
access fault, which ends THIS process, not the test session.  An engine per case, as in the other guard children: every buffer then
has exactly the case's size.  Prints one line `TSDF_GUARD_OK <cases>` when everything ran and matched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import tsdf_ref as TR
    from stereo_reconstruction_cv_amd.stereo import Engine
    u32 = lambda a: np.ascontiguousarray(a).view(np.uint32)
    ncase = 0
    for case in TR.cases():
        e = Engine(dict(numDisparities=16))
        a, b = TR.case_input(case), TR.case_input(case, seed=5)
        want = TR.empty(a["dims"], a["colors"] is not None)
        got = TR.empty(a["dims"], a["colors"] is not None)
        for f in (a, b):
            st_w = TR.run_case(f, want)[1]
            st = e.tsdf_integrate_host(f["dims"], f["vs"], f["tau"], f["origin"], got[0], got[1], got[2], f["xyz"], f["disp"], f["colors"],
                                       f["cam"], f["front"], f["ext"], stats=True)
            assert st.tolist() == st_w.tolist(), (case, st, st_w)
            assert all(x is None or np.array_equal(x, y) for x, y in zip(got, want)), case
        wp, wc = TR.extract(a["dims"], a["vs"], a["origin"], *want, 1)
        n = wp.shape[0]
        for cap in sorted({0, max(n - 1, 0), n, n + 3}):
            pts = np.full((cap, 3), 7, np.float32)
            col = np.full((cap, 3), 7, np.uint8) if wc is not None else None
            total = e.tsdf_extract_host(a["dims"], a["vs"], a["origin"], got[0], got[1], got[2], 1, pts if cap else None, col if cap else None)
            k = min(n, cap)
            assert total == n and np.array_equal(u32(pts[:k]), u32(wp[:k])) and (pts[k:] == 7).all(), (case, cap, total, n)
            assert wc is None or (np.array_equal(col[:k], wc[:k]) and (col[k:] == 7).all()), (case, cap)
        ncase += 1
    print(f"TSDF_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
