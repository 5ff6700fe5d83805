"""Child process of tests/test_gpu_icp.py: some of its shapes and a few of its extremes once under the engine's GUARDED allocation
mode (SGM_DEBUG_ALLOC=1, sgm_engine.hip: DevBuf::ensure_guarded; why: tests/guard_child.py).  The staged source and target, the
target's table and sorted records, the correspondences, the squared distances and the blocks' partial sums end where their mappings
end, so a run read past a cell (rad_walk under k_icp_correspond, whose query point is no record of the grid), a partner index past
the target (k_icp_terms), a lane past ns or a record past the blocks (k_icp_reduce) dies here with a memory access fault, which ends
THIS process, not the test session.  An engine per case, as in the other guard children: every buffer then has exactly the case's
size.  Prints one line `ICP_GUARD_OK <cases>` when everything ran and matched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402


def main():
    assert os.environ.get("SGM_DEBUG_ALLOC") == "1"
    import icp_ref as IR
    from stereo_reconstruction_cv_amd.stereo import Engine
    u32 = lambda a: np.ascontiguousarray(a).view(np.uint32)
    u64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)

    def check(src, ds, tgt, dt, tn, r, est, maxit, want=None):
        e = Engine(dict(numDisparities=16))
        if want is None:
            want = IR.register(src, ds, tgt, dt, tn, r, estimation=est, max_iteration=maxit)
        T, fit, rmse, corr, d2, hist, st = e.register_icp_host(src, ds, tgt, dt, tn, r, (0, 0, 0), None, est, maxit)
        assert st.tolist() == want["stats"].tolist(), (st, want["stats"])
        assert u64(T).tolist() == u64(want["T"]).tolist() and (fit, rmse) == (want["fitness"], want["rmse"])
        assert np.array_equal(corr, want["corr"]) and np.array_equal(u32(d2), u32(want["d2"]))
        assert u64(hist).tolist() == u64(want["history"]).tolist()
        moved, _ = e.transform_points_host(np.asarray(src, np.float32).reshape(-1, 3), T)
        assert np.array_equal(u32(moved), u32(IR.transform(IR.m_of(T), np.asarray(src, np.float32).reshape(-1, 3))))

    ncase = 0
    for (ns, nt), with_disp, est in (((1, 1), True, 0), ((63, 300), True, 1), ((64, 5000), False, 1), ((65, 1), True, 1), ((255, 300), False, 0),
                                     ((256, 5000), True, 1), ((257, 300), True, 1), ((1000, 5000), True, 0), ((1000, 1), False, 1),
                                     ((65537, 300), True, 1)):
        i = IR.SHAPE_CASES.index((ns, nt))
        src, ds, tgt, dt, tn = IR.case_input(i)
        check(src, ds if with_disp else None, tgt, dt if with_disp else None, tn, IR.R_CASE, est, IR.SHAPE_ITERATIONS,
              IR.case_want(i, with_disp, est))
        ncase += 1
    src, _, tgt, _, tn, r = IR.condition_case("tie")
    check(src, None, tgt, None, None, r, 0, 0)
    src, _, tgt, _, tn, r = IR.condition_case("plane")
    check(src, None, tgt, None, tn, r, 1, 5)
    src, ds, tgt, dt, tn = IR.case_input(IR.SHAPE_CASES.index((257, 300)))
    check(np.full_like(src, np.nan), None, tgt, dt, tn, IR.R_CASE, 1, 2)            # nothing valid
    check(src, ds, np.zeros((0, 3), np.float32), None, None, IR.R_CASE, 0, 2)        # no target
    ncase += 4
    print(f"ICP_GUARD_OK {ncase}", flush=True)


if __name__ == "__main__":
    main()
