#!/usr/bin/env python3
"""Per-stage HIP-event timings of a colour pair (SGM_OPT_CHANNELS = 3) beside the gray pair it is made from, device
pointers, both schedules of the single-pair path; then the throughput-mode batch entry with N colour pairs.
    tools/color_stages.py [H W D bs mode [N]]        (default: 4K D=256 bs=7 MODE_HH, N = 8)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import stereo_reconstruction_cv_amd as cv  # noqa: E402
from stereo_reconstruction_cv_amd import _lib, synth  # noqa: E402

a = sys.argv[1:]
H, W, D, bs, mode = (int(v) for v in (a[:5] if len(a) >= 5 else (2160, 3840, 256, 7, 1)))
N = int(a[5]) if len(a) > 5 else 8
l, r, _ = synth.make_pair(H, W, D, 1234)
l2, r2, _ = synth.make_pair(H, W, D, 4321)
l3, r3 = np.stack([l, l2, l[::-1]], axis=2), np.stack([r, r2, r[::-1]], axis=2)   # three different textures, one shift
gray = (torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda(), 1)
colour = (torch.from_numpy(np.ascontiguousarray(l3)).cuda(), torch.from_numpy(np.ascontiguousarray(r3)).cuda(), 3)
out = torch.empty((H, W), dtype=torch.int16, device="cuda")
for sched in (1, 2):
    for name, (dl, dr, cn) in (("gray", gray), ("colour", colour)):
        eng = cv.Engine(bench.sgbm_params(D, bs, mode))
        eng.set_option(_lib.SGM_OPT_PROFILE, 1)
        eng.set_option(_lib.SGM_OPT_SCHEDULE, sched)
        for _ in range(5):
            eng.compute_device(dl.data_ptr(), dr.data_ptr(), H, W, cn * W, out.data_ptr(), cn)
            st = eng.stage_times()
        print(f"{H}x{W} D={D} bs={bs} mode {mode} sched {sched} {name:6s}: wall {dict((n, m) for n, m, _ in st)['_wall']:.2f} ms  "
              + " ".join(f"{n}={m:.2f}" for n, m, _ in st if n != "_wall" and m > 0.02)
              + f"  headroom ok={eng.headroom()['ok']}", flush=True)
        del eng
        torch.cuda.empty_cache()
# throughput mode: N pairs resident, chained groups
for name, (dl, dr, cn) in (("gray", gray), ("colour", colour)):
    eng = cv.Engine(bench.sgbm_params(D, bs, mode))
    eng.set_option(_lib.SGM_OPT_SCHEDULE, 2)
    outs = [torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(N)]
    ts = []
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.pipeline_batch_device([dl.data_ptr()] * N, [dr.data_ptr()] * N, H, W, cn * W, None, [o.data_ptr() for o in outs], cn=cn)
        eng.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / N)
    print(f"batch of {N} {name:6s}, throughput mode: {min(ts):.2f} ms per pair (best of 3; {' '.join(f'{t:.2f}' for t in ts)})", flush=True)
    eng.trim()
    del eng
    torch.cuda.empty_cache()
