#!/usr/bin/env python3
"""Timings of the wide disparity ranges (numDisparities > 512: NP = 8, one path kernel per direction) on the
GPU box: per-stage HIP-event times, ms per pair and achieved bytes/s against the unfused traffic model of the route.

    tools/wide_d_times.py [reps [out.json]]        reps: timed repetitions after 2 warm-up computes, default 5

Workloads: 4K D = 1024 in modes 0, 1, 3; 4K D = 768 mode 1; 1080p D = 1024 mode 1; and, as the consistency figure,
4K D = 512 mode 1 with SGM_OPT_SCHEDULE 0 -- the same kernels at NP = 4.  Inputs are device-resident; blockSize 7 and the
penalties of bench.py.

Traffic model (V = 2 H W1 D bytes): the int16 cost stage moves about 3.1 V (k_hsum writes V; the vertical sum reads it
once plus the window overlap of its bands and writes V); a path kernel reads C and S and writes S = 3 V, less the S read
of the first direction (S = L) and the S write of the last (the winner-take-all is fused, S is not kept)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import stereo_reconstruction_cv_amd as cv  # noqa: E402
from stereo_reconstruction_cv_amd import _lib, synth  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else None
NDIR = {0: 5, 1: 8, 3: 4}
WORK = [(2160, 3840, 1024, 0, 1), (2160, 3840, 1024, 1, 1), (2160, 3840, 1024, 3, 1), (2160, 3840, 768, 1, 1), (1080, 1920, 1024, 1, 1),
        (2160, 3840, 512, 1, 0)]
results = []
for H, W, D, mode, sched in WORK:
    l, r, _ = synth.make_pair(H, W, D, 1234)
    dl, dr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
    out = torch.empty((H, W), dtype=torch.int16, device="cuda")
    eng = cv.Engine(bench.sgbm_params(D, 7, mode))
    eng.set_option(_lib.SGM_OPT_PROFILE, 1)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, sched)
    totals, walls, stages = [], [], {}
    for it in range(2 + reps):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.compute_device(dl.data_ptr(), dr.data_ptr(), H, W, W, out.data_ptr())
        eng.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        st = eng.stage_times()
        if it >= 2:
            walls.append(dt)
            totals.append(sum(m for n, m, _ in st if n != "_wall"))
            for n, m, _ in st:
                stages.setdefault(n, []).append(m)
    hr = eng.headroom()
    _, W1 = eng.geometry(W)
    V = 2 * H * W1 * D
    cost_v = 3.1 if not any(n == "cost_box" for n in stages) else 2.05      # (the D = 512 row takes the byte pipeline)
    model_v = cost_v + 3 * NDIR[mode] - 2
    ms = statistics.median(totals)
    path_ms = sum(statistics.median(v) for n, v in stages.items() if n.startswith("path"))
    free, total = torch.cuda.mem_get_info()
    rec = dict(H=H, W=W, D=D, mode=mode, schedule=sched, W1=W1, volume_bytes=V, ms_per_pair=round(ms, 3), ms_min=round(min(totals), 3),
               ms_max=round(max(totals), 3), host_wall_ms=round(statistics.median(walls), 3), model_volumes=round(model_v, 2),
               model_bytes=int(model_v * V), achieved_TBps=round(model_v * V / (ms * 1e-3) / 1e12, 3),
               path_ms=round(path_ms, 3), path_TBps=round((3 * NDIR[mode] - 2) * V / (path_ms * 1e-3) / 1e12, 3),
               ms_per_volume_GB=round(ms / (V / 1e9), 4), device_GiB=round((total - free) / 2**30, 2), headroom=hr,
               valid_fraction=round(float((out >= 0).float().mean()), 4),
               stages={n: round(statistics.median(v), 3) for n, v in stages.items()})
    results.append(rec)
    print(json.dumps(rec), flush=True)
    del eng, dl, dr, out
    torch.cuda.empty_cache()
wide = next(x for x in results if x["D"] == 1024 and x["mode"] == 1 and x["H"] == 2160)
ref = next(x for x in results if x["D"] == 512)
ratio = dict(ms_per_volume_byte_D1024_over_D512_schedule0=round(wide["ms_per_volume_GB"] / ref["ms_per_volume_GB"], 3),
             path_ms_per_volume_byte_ratio=round((wide["path_ms"] / wide["volume_bytes"]) / (ref["path_ms"] / ref["volume_bytes"]), 3))
print(json.dumps(ratio), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(dict(reps=reps, workloads=results, consistency=ratio), f, indent=1)
