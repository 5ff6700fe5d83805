"""Child process of tests/test_gpu_voxel.py: a dozen of its cases once under the engine's GUARDED allocation mode
(SGM_DEBUG_ALLOC=1, sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py).  The staged points, disparities and
colours, the per-point slot words, the block counts, the three outputs and the hash table end where their mappings end, so a probe
that leaves the table (k_voxel_insert), a slot word or a block count stored past its array, or an output row written past the
voxels' number (k_voxel_scatter) dies here with a memory access fault, which ends THIS process, not the test session.  An engine
per case, as in the other guard children: every buffer then has exactly the case's size.  Prints one line `VOXEL_GUARD_OK <cases>`
when everything ran and matched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import voxel_ref as VR
    from stereo_reconstruction_cv_amd import _lib
    from stereo_reconstruction_cv_amd.stereo import Engine

    def check(e, xyz, disp, col, v, o, mp, want=None):
        if want is None:
            want = VR.voxel_downsample(xyz, disp, col, v, o, mp)
        p, c, k, noor = e.voxel_downsample_host(xyz, disp, col, v, o, mp, return_counts=True)
        assert p.shape[0] == want["n_voxels"] and noor == want["n_out_of_range"], (p.shape, want["n_voxels"], noor)
        assert np.array_equal(p.view(np.uint32), want["points"].view(np.uint32)) and np.array_equal(k, want["counts"])
        assert col is None or np.array_equal(c, want["colors"])

    ncase = 0
    for i, (H, W, v, o, mp) in enumerate(VR.SHAPE_CASES):            # six shapes
        xyz, disp, col = VR.case_input(i)
        check(Engine(dict(numDisparities=16)), xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3), v, o, mp, VR.case_want(i))
        ncase += 1
    xyz, disp, col = VR.layered_cloud(48, 320, 704)
    xyz, disp, col = xyz.reshape(-1, 3), disp.reshape(-1), col.reshape(-1, 3)
    far = xyz.copy()
    far[5::7, 0] = 3.0e5
    g = np.stack(np.meshgrid(np.arange(64), np.arange(64), indexing="ij"), axis=2).reshape(-1, 2)
    own = np.concatenate([g, (g[:, :1] * 7 + g[:, 1:]) % 5], axis=1).astype(np.float32) + np.float32(0.5)
    for debug, pts, d, c, v, o, mp in (
            (0, xyz, disp, col, 1.0e6, (-5.0e5,) * 3, 1),           # one voxel
            (0, xyz, disp, col, 1.0e-5, (0, 0, 0), 1),              # a voxel per point
            (0, xyz, np.zeros_like(disp), col, 0.05, (0, 0, 0), 1),  # nothing valid
            (0, far, disp, None, 0.05, (0, 0, 0), 1),               # out-of-range points among the others
            (0, xyz, None, col, 0.05, (0.013, -2.5, 100.0), 5),     # no disparities, an origin, a floor on the count
            (_lib.SGM_DBG_VOXEL_TIGHT_TABLE, own, None, None, 1.0, (0, 0, 0), 1),                    # load 1.0
            (_lib.SGM_DBG_VOXEL_TIGHT_TABLE, xyz, disp, col, 0.05, (0, 0, 0), 1),
            (_lib.SGM_DBG_VOXEL_OTHER_REDUCTION, xyz, disp, col, 0.05, (0, 0, 0), 2)):
        e = Engine(dict(numDisparities=16))
        e.set_option(_lib.SGM_OPT_DEBUG, debug)
        check(e, pts, d, c, v, o, mp)
        ncase += 1
    print(f"VOXEL_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
