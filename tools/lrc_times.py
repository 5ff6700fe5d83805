#!/usr/bin/env python3
"""What the left-right consistency confidence costs, on the GPU box, in ONE run:

  1. sgm_lrc_confidence_device on one pair of maps at 4K, 1080p and 720p (radius 5, the default without a matcher; at 4K also
     radius 16), left confidence with a base map, next to the edge-aware filter on the same map in the same engine;
  2. sgm_lrc_confidence_batch_device at 17 x 4K, 32 x 1080p and 64 x 720p, per pair;
  3. computeFiltered on a device-resident 4K D = 256 MODE_HH pair and computeFilteredBatch on 4 x 1080p D = 128 pairs under
     confidence = "margin" (the path before this stage existed), "lrc" and "both", alternating, host wall clock around calls that
     end in a synchronise: what the extra right-view pass and this stage add to the parent's path.

    tools/lrc_times.py [reps [out.json]]        (default output: profiles/lrc/times.json)

SGM_OPT_PROFILE is on for 1 and 2 (HIP events around each stage), two warm-up calls, median of `reps`; `model_bytes` is what the
two kernels must move (maps 2 x 2 bytes and factor planes 2 x 1 byte through k_lrc_factor; maps, planes, base and the result
through k_lrc_match), `GBps` that over the stage total.  The maps are synthetic: three levels in blocks with noise and 10 % holes,
the right map another draw of the same; the kernels' time does not follow the content beyond the share of invalid pixels."""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lrc", "times.json")
SIZES = [("4K", 2160, 3840), ("1080p", 1080, 1920), ("720p", 720, 1280)]
med = lambda v: round(statistics.median(v), 4)
ptr = lambda ts: [t.data_ptr() for t in ts]


def maps(H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    layer = (torch.arange(H, device="cuda")[:, None] // 97 + torch.arange(W, device="cuda")[None, :] // 131) % 3
    level = torch.tensor([200, 420, 600], device="cuda")[layer]
    out = []
    for _ in range(2):
        d = (level + torch.randint(-6, 7, (H, W), device="cuda", generator=g)).to(torch.int16)
        d[torch.rand((H, W), device="cuda", generator=g) < 0.1] = -16
        out.append(d.contiguous())
    return out[0], out[1], torch.randint(0, 101, (H, W), device="cuda", generator=g, dtype=torch.uint8)


def stage_sums(e):
    return {n: m for n, m, _ in e.stage_times() if n != "_wall"}


results = dict(reps=reps, single=[], batch=[], filtered=[])
lut = cv.wls_weights(1.5)

# ---- 1. one pair ----------------------------------------------------------------------------------------------------------------
for name, H, W in SIZES:
    dl, dr, base = maps(H, W, 1)
    guide = torch.randint(0, 256, (H, W), device="cuda", dtype=torch.uint8)
    cl = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    out = torch.empty((H, W), dtype=torch.int16, device="cuda")
    e = cv.Engine(dict(numDisparities=16))
    e.set_option(_lib.SGM_OPT_PROFILE, 1)
    for r in ((5, 16) if name == "4K" else (5,)):
        lrc, wls, wall = [], [], []
        for it in range(2 + reps):
            e.synchronize()
            t0 = time.perf_counter()
            e.lrc_confidence_device(dl.data_ptr(), dr.data_ptr(), base.data_ptr(), H, W, -16, 24, r, 2304, cl.data_ptr())
            e.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            a = stage_sums(e)
            e.wls_filter_device(dl.data_ptr(), guide.data_ptr(), 1, cl.data_ptr(), H, W, -16, 8000.0, lut, out.data_ptr())
            b = stage_sums(e)
            if it >= 2:
                lrc.append(a)
                wls.append(sum(b.values()))
                wall.append(dt)
        st = {n: med([x[n] for x in lrc]) for n in lrc[0]}
        total = med([sum(x.values()) for x in lrc])
        npx = H * W
        model = npx * (4 + 2) + npx * (4 + 2 + 1 + 1)
        rec = dict(size=name, H=H, W=W, radius=r, stages_ms=st, ms=total, host_wall_ms=med(wall), filter_ms=med(wls),
                   share_of_filter=round(total / med(wls), 4), model_bytes=model, GBps=round(model / (total * 1e-3) / 1e9, 1),
                   nonzero_fraction=round(float((cl != 0).float().mean()), 4))
        results["single"].append(rec)
        print(json.dumps(rec), flush=True)
    del e

# ---- 2. batches -------------------------------------------------------------------------------------------------------------------
for (name, H, W), N in zip(SIZES, (17, 32, 64)):
    src = [maps(H, W, 10 + k) for k in range(3)]
    which = [k % 3 for k in range(N)]
    cls = [torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(N)]
    e = cv.Engine(dict(numDisparities=16))
    e.set_option(_lib.SGM_OPT_PROFILE, 1)
    lrc, wall = [], []
    for it in range(2 + reps):
        e.synchronize()
        t0 = time.perf_counter()
        e.lrc_confidence_batch_device([src[k][0].data_ptr() for k in which], [src[k][1].data_ptr() for k in which],
                                      [src[k][2].data_ptr() for k in which], H, W, -16, 24, 5, 2304, ptr(cls))
        e.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        if it >= 2:
            lrc.append(stage_sums(e))
            wall.append(dt)
    total = med([sum(x.values()) for x in lrc])
    npx = H * W
    model = N * (npx * (4 + 2) + npx * (4 + 2 + 1 + 1))
    rec = dict(size=name, H=H, W=W, N=N, radius=5, stages_ms={n: med([x[n] for x in lrc]) for n in lrc[0]}, ms=total,
               ms_per_pair=round(total / N, 4), host_wall_ms_per_pair=round(med(wall) / N, 4), model_bytes=model,
               GBps=round(model / (total * 1e-3) / 1e9, 1))
    results["batch"].append(rec)
    print(json.dumps(rec), flush=True)
    e.trim()
    del e, src, cls
    torch.cuda.empty_cache()

# ---- 3. computeFiltered under the three confidence sources ----------------------------------------------------------------------
for name, H, W, D, mode, N in (("4K D256 HH", 2160, 3840, 256, 1, 1), ("1080p D128 SGBM batch of 4", 1080, 1920, 128, 0, 4)):
    pairs = [synth.make_pair(H, W, D, 1234 + i)[:2] for i in range(N)]
    L = [torch.from_numpy(a).cuda() for a, _ in pairs]
    R = [torch.from_numpy(b).cuda() for _, b in pairs]
    m = cv.StereoSGBM_create(**bench.sgbm_params(D, 7, mode))
    walls = {s: [] for s in ("margin", "lrc", "both")}
    for it in range(2 + reps):
        for source in walls:                               # alternating: the three settings see the same minute of the machine
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = m.computeFiltered(L[0], R[0], confidence=source) if N == 1 else m.computeFilteredBatch(L, R, confidence=source)
            torch.cuda.synchronize()
            if it >= 2:
                walls[source].append((time.perf_counter() - t0) * 1e3 / N)
    rec = dict(workload=name, H=H, W=W, D=D, mode=mode, pairs_per_call=N,
               host_wall_ms_per_pair={s: med(v) for s, v in walls.items()},
               spread={s: [round(min(v), 3), round(max(v), 3)] for s, v in walls.items()})
    rec["lrc_minus_margin_ms"] = round(rec["host_wall_ms_per_pair"]["lrc"] - rec["host_wall_ms_per_pair"]["margin"], 3)
    rec["both_minus_margin_ms"] = round(rec["host_wall_ms_per_pair"]["both"] - rec["host_wall_ms_per_pair"]["margin"], 3)
    results["filtered"].append(rec)
    print(json.dumps(rec), flush=True)
    del L, R, m
    cv.clear_engine_cache()
    torch.cuda.empty_cache()

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
