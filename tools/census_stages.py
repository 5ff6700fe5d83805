#!/usr/bin/env python3
"""Per-stage HIP-event timings of one gray pair under the Birchfield-Tomasi cost and under the census cost (SGM_OPT_COST),
device pointers, both schedules of the single-pair path; then the throughput-mode batch entry with N pairs under either cost.
A trailing debug mask goes to SGM_OPT_DEBUG (4: the wave form of k_pix_census at D <= 32; 256: the int16 box route).
    tools/census_stages.py [H W D bs mode [N [debug]]]        (default: 4K D=256 bs=7 MODE_HH, N = 8)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import stereo_reconstruction_cv_amd as cv  # noqa: E402
from stereo_reconstruction_cv_amd import _lib, synth  # noqa: E402

a = sys.argv[1:]
H, W, D, bs, mode = (int(v) for v in (a[:5] if len(a) >= 5 else (2160, 3840, 256, 7, 1)))
N = int(a[5]) if len(a) > 5 else 8
debug = int(a[6]) if len(a) > 6 else 0
COSTS = (("BT", _lib.SGM_COST_BT), ("census", _lib.SGM_COST_CENSUS))
COST_STAGES = ("features", "cost_pix", "census", "cost_pix_census", "cost_box", "cost_hsum", "cost_vsum")
l, r, _ = synth.make_pair(H, W, D, 1234)
dl, dr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
out = torch.empty((H, W), dtype=torch.int16, device="cuda")
for sched in (1, 2):
    for name, cost in COSTS:
        eng = cv.Engine(bench.sgbm_params(D, bs, mode))
        eng.set_option(_lib.SGM_OPT_PROFILE, 1)
        eng.set_option(_lib.SGM_OPT_SCHEDULE, sched)
        eng.set_option(_lib.SGM_OPT_COST, cost)
        if debug:
            eng.set_option(_lib.SGM_OPT_DEBUG, debug)
        best = None
        for _ in range(6):
            eng.compute_device(dl.data_ptr(), dr.data_ptr(), H, W, W, out.data_ptr())
            st = eng.stage_times()
            cs = sum(m for n, m, _ in st if n in COST_STAGES)
            if best is None or cs < best[0]:
                best = (cs, st)
        cs, st = best
        print(f"{H}x{W} D={D} bs={bs} mode {mode} sched {sched} dbg {debug} {name:6s}: cost stages {cs:.3f} ms  wall {dict((n, m) for n, m, _ in st)['_wall']:.2f} ms  "
              + " ".join(f"{n}={m:.3f}" for n, m, _ in st if n != "_wall" and (m > 0.02 or n in COST_STAGES))
              + f"  headroom ok={eng.headroom()['ok']}", flush=True)
        del eng
        torch.cuda.empty_cache()
# throughput mode: N pairs resident, chained groups
for name, cost in COSTS:
    eng = cv.Engine(bench.sgbm_params(D, bs, mode))
    eng.set_option(_lib.SGM_OPT_SCHEDULE, 2)
    eng.set_option(_lib.SGM_OPT_COST, cost)
    outs = [torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(N)]
    ts = []
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.pipeline_batch_device([dl.data_ptr()] * N, [dr.data_ptr()] * N, H, W, W, None, [o.data_ptr() for o in outs])
        eng.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / N)
    print(f"batch of {N} {name:6s}, throughput mode: {min(ts):.2f} ms per pair (best of 3; {' '.join(f'{t:.2f}' for t in ts)})", flush=True)
    eng.trim()
    del eng
    torch.cuda.empty_cache()
