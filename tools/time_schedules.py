#!/usr/bin/env python3
"""Per-stage HIP-event timings of the schedules and the modes at a given shape, and the throughput-mode batch (GPU box).

    tools/time_schedules.py [H W D bs [schedules [modes [reps [batch]]]]]
        schedules  comma list, default 0,1        modes  comma list of 0 (MODE_SGBM), 1 (MODE_HH), 3 (MODE_HH4), default 0,1,3
        reps       timed repetitions after 2 warm-up computes, default 5 (the median and the spread are printed)
        batch      pairs of a resident throughput-mode batch (SGM_OPT_SCHEDULE 2), wall clock per pair; default 0 = none

A library that lacks a mode (SGM_HIP_LIB pointing at an older build) reports it and goes on with the next."""
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

a = sys.argv[1:]
H, W, D, bs = (int(v) for v in (a[:4] if len(a) >= 4 else (2160, 3840, 256, 7)))
scheds = [int(v) for v in a[4].split(",")] if len(a) > 4 and a[4] else [0, 1]
modes = [int(v) for v in a[5].split(",")] if len(a) > 5 else [0, 1, 3]
reps = int(a[6]) if len(a) > 6 else 5
nbatch = int(a[7]) if len(a) > 7 else 0
l, r, _ = synth.make_pair(H, W, D, 1234)
dl, dr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
out = torch.empty((H, W), dtype=torch.int16, device="cuda")


def med(v):
    return f"{statistics.median(v):.2f} [{min(v):.2f} .. {max(v):.2f}]"


for mode in modes:
    for sched in scheds:
        try:
            eng = cv.Engine(bench.sgbm_params(D, bs, mode))
        except cv.error as e:
            print(f"mode {mode}: {e}", flush=True)
            break
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
        free, total = torch.cuda.mem_get_info()
        print(f"{H}x{W} D={D} mode {mode} sched {sched}: stages {med(totals)} ms, host wall {med(walls)} ms, device memory in use {(total - free) / 2**30:.2f} GiB  "
              + " ".join(f"{n}={statistics.median(v):.2f}" for n, v in stages.items() if statistics.median(v) > 0.25), flush=True)
        del eng
    if nbatch:
        try:
            eng = cv.Engine(bench.sgbm_params(D, bs, mode))
        except cv.error:
            continue
        eng.set_option(_lib.SGM_OPT_SCHEDULE, 2)
        dd = [torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(nbatch)]
        pl, pr, pd = [dl.data_ptr()] * nbatch, [dr.data_ptr()] * nbatch, [t.data_ptr() for t in dd]
        per = []
        for it in range(2 + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.pipeline_batch_device(pl, pr, H, W, W, None, pd)
            eng.synchronize()
            if it >= 2:
                per.append((time.perf_counter() - t0) * 1e3 / nbatch)
        eng.check()
        free, total = torch.cuda.mem_get_info()
        same = all(torch.equal(dd[0], t) for t in dd[1:])
        print(f"{H}x{W} D={D} mode {mode} throughput mode, {nbatch} resident pairs: {med(per)} ms per pair; device memory in use "
              f"{(total - free) / 2**30:.2f} GiB; maps identical: {same}", flush=True)
        del eng, dd
        torch.cuda.empty_cache()
