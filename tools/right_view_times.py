#!/usr/bin/env python3
"""What SGM_OPT_RIGHT_VIEW costs, on the GPU box: every workload with the option off and on in the same
build, alternating on ONE engine, device-resident synthetic pairs, blockSize 7 and the penalties of bench.py (the notebook's
D = 16 row: blockSize 11), SGM_OPT_PROFILE, two warm-up computes, median of 5.

    tools/right_view_times.py [reps [out.json]]        (default output: profiles/right_view/times.json)

Per workload and setting: ms per pair (sum of the stage times of a single pair; host wall clock over the whole call for the
batch of 17, whose pairs run on internal engines), the stage breakdown, and `on - off` per stage, so that the row says which
kernel carries the difference.  The bar: the option replaces a second compute on the flipped, swapped pair, so `on_over_2off`
= t_on / (2 t_off) must be clearly below 1.  `right_wta_GBps`: the model's bytes of the diagonal pass -- one read of every
volume the winner-take-all adds up, V = 2 H W1 D bytes each -- over the time of its stage.  `diverted`: the configuration
fuses its winner-take-all into the last path kernel by default and runs it as a pass of its own with the option on (the
last path kernel then also writes S and k_wta_t reads it back: 2 V more, as for the confidence option)."""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "right_view", "times.json")
# (name, H, W, D, blockSize, mode, schedule, pairs per call)
WORK = [("4K D256 HH alone", 2160, 3840, 256, 7, 1, 1, 1), ("4K D256 HH batch of 17", 2160, 3840, 256, 7, 1, 2, 17),
        ("4K D256 SGBM", 2160, 3840, 256, 7, 0, 1, 1), ("4K D16 bs11 SGBM", 2160, 3840, 16, 11, 0, 1, 1),
        ("720p D64 SGBM", 720, 1280, 64, 7, 0, 1, 1), ("4K D1024 HH", 2160, 3840, 1024, 7, 1, 1, 1)]
results = []
for name, H, W, D, bs, mode, sched, N in WORK:
    pairs = [synth.make_pair(H, W, D, 1234 + i)[:2] for i in range(min(N, 3))]
    dl = [torch.from_numpy(pairs[i % len(pairs)][0]).cuda() for i in range(N)]
    dr = [torch.from_numpy(pairs[i % len(pairs)][1]).cuda() for i in range(N)]
    dd = [torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(N)]
    dc = [torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(N)]
    p = bench.sgbm_params(D, bs, mode)
    # ONE engine, the option toggled between calls (the engines behind a batch inherit it per call): two engines with a
    # group of 17 4K pairs each would not fit in device memory side by side
    e = cv.Engine(p)
    e.set_option(_lib.SGM_OPT_PROFILE, 1)
    e.set_option(_lib.SGM_OPT_SCHEDULE, sched)
    ptr = lambda ts: [t.data_ptr() for t in ts]
    walls, totals, stages = {0: [], 1: []}, {0: [], 1: []}, {0: {}, 1: {}}
    for it in range(2 + reps):
        for on in (0, 1):                               # alternating: both settings see the same minute of the machine
            e.set_option(_lib.SGM_OPT_RIGHT_VIEW, on)
            e.synchronize()
            t0 = time.perf_counter()
            if N == 1:
                e.compute_device(dl[0].data_ptr(), dr[0].data_ptr(), H, W, W, dd[0].data_ptr(), d_rmap=dc[0].data_ptr() if on else None)
            else:
                e.pipeline_batch_device(ptr(dl), ptr(dr), H, W, W, None, ptr(dd), d_rmaps=ptr(dc) if on else None)
            e.synchronize()
            dt = (time.perf_counter() - t0) * 1e3 / N
            st = e.stage_times()
            if it >= 2:
                walls[on].append(dt)
                totals[on].append(sum(m for n, m, _ in st if n != "_wall"))
                for n, m, _ in st:
                    stages[on].setdefault(n, []).append(m)
    med = lambda v: round(statistics.median(v), 3)
    _, W1 = e.geometry(W)
    V = 2 * H * W1 * D
    s_off = {n: med(v) for n, v in stages[0].items()}
    s_on = {n: med(v) for n, v in stages[1].items()}
    diverted = not any(n == "wta" for n in s_off)
    nvol = _lib.debug_plan(p, H, W, 1, sched, right_view=1)["nvol"]
    rec = dict(workload=name, H=H, W=W, D=D, blockSize=bs, mode=mode, schedule=sched, pairs_per_call=N, volume_bytes=V,
               ms_per_pair_off=med(totals[0]) if N == 1 else med(walls[0]), ms_per_pair_on=med(totals[1]) if N == 1 else med(walls[1]),
               host_wall_ms_per_pair_off=med(walls[0]), host_wall_ms_per_pair_on=med(walls[1]),
               spread_off=[round(min(walls[0]), 3), round(max(walls[0]), 3)], spread_on=[round(min(walls[1]), 3), round(max(walls[1]), 3)],
               diverted=diverted, volumes_read=nvol, extra_bytes_model=(2 * V if diverted else 0) + nvol * V + 8 * H * W1 * 2 + 6 * H * W,
               stages_off=s_off, stages_on=s_on,
               stage_delta={n: round(s_on.get(n, 0.0) - s_off.get(n, 0.0), 3) for n in sorted(set(s_on) | set(s_off)) if n != "_wall"},
               right_valid_fraction=round(float((dc[0] != -16).float().mean()), 4), headroom=e.headroom())
    rec["delta_ms_per_pair"] = round(rec["ms_per_pair_on"] - rec["ms_per_pair_off"], 3)
    rec["on_over_2off"] = round(rec["ms_per_pair_on"] / (2 * rec["ms_per_pair_off"]), 3)
    if N == 1 and s_on.get("right_wta"):
        rec["right_wta_GBps"] = round(nvol * V / (s_on["right_wta"] * 1e-3) / 1e9, 1)
        if s_on.get("wta"):
            rec["wta_GBps"] = round(nvol * V / (s_on["wta"] * 1e-3) / 1e9, 1)
    results.append(rec)
    print(json.dumps(rec), flush=True)
    del e, dl, dr, dd, dc
    torch.cuda.empty_cache()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(dict(reps=reps, workloads=results), f, indent=1)
