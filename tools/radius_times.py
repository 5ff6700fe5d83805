#!/usr/bin/env python3
"""What the radius outlier removal costs, on the GPU box, in ONE run:

  for the device-resident XYZ image of a synthetic 4K D = 256 MODE_HH pair, and of a 1080p D = 128 and a 720p D = 64 pair
  (sgm_pipeline_device with the default Q), sgm_radius_outlier_device with every output at three radii found by bisection on the
  counts output so that the mean neighbour count of the points in range is about 4, 20 and 100 -- each with
  max_count = nb_points = 8 (the search stops at 8) and with max_count = 2^24 - 1 (the full count), and each in the four
  combinations of the query order (sorted by cell, the default; source order, SGM_DBG_RADIUS_SOURCE_ORDER) and the table size
  (twice the points, the default; tight, SGM_DBG_RADIUS_TIGHT_TABLE), alternating; beside them, in the same run,
  sgm_voxel_downsample_device at voxel_size = radius and sgm_compact_points_device on the same cloud, and the pair's own compute.

    tools/radius_times.py [reps [out.json]]        (default output: profiles/radius/times.json)

Times are host wall clock around calls that end in a synchronise (the entries block for their counts), two warm-up calls, median
of `reps` with the spread; with SGM_OPT_PROFILE on in a second pass the stage record (HIP events) splits a call into radius_count /
radius_clear / radius_insert / radius_starts / radius_sort / radius_query / radius_compact.  `table_MB` is the table the call
clears: 16 bytes per slot, the smallest power of two of at least twice the points in range."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import stereo_reconstruction_cv_amd as cv  # noqa: E402
from stereo_reconstruction_cv_amd import _lib, synth  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "radius", "times.json")
SIZES = [("4K D256 HH", 2160, 3840, 256, 1), ("1080p D128 HH", 1080, 1920, 128, 1), ("720p D64 HH", 720, 1280, 64, 1)]
TARGETS = (4, 20, 100)
FULL = (1 << 24) - 1
TIGHT, SOURCE = _lib.SGM_DBG_RADIUS_TIGHT_TABLE, _lib.SGM_DBG_RADIUS_SOURCE_ORDER
VARIANTS = (("sorted", 0), ("source", SOURCE), ("sorted_tight", TIGHT), ("source_tight", SOURCE | TIGHT))
MODES = (("stop_at_8", 8, 8), ("full_count", 8, FULL))
med = lambda v: round(statistics.median(v), 4)
spread = lambda v: [round(min(v), 4), round(max(v), 4)]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


results = dict(reps=reps, library_default="sorted", clouds=[])
for name, H, W, D, mode in SIZES:
    a, b = synth.make_pair(H, W, D, 1234)[:2]
    e = cv.Engine(bench.sgbm_params(D, 7, mode))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    n = H * W
    dd = torch.empty((H, W), dtype=torch.int16, device="cuda")
    df = torch.empty((H, W), dtype=torch.float32, device="cuda")
    dx = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    rgb = torch.from_numpy(np.ascontiguousarray(np.repeat(a[:, :, None], 3, axis=2))).cuda()
    pts = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    oc = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    Q = synth.default_Q(W)

    def compute():
        e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, Q, dd.data_ptr(), df.data_ptr(), dx.data_ptr())
        e.synchronize()

    def compact():
        return e.compact_points_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), n, pts.data_ptr(), oc.data_ptr())

    def voxel(v):
        return e.voxel_downsample_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), n, v, (0.0, 0.0, 0.0), 1, pts.data_ptr(), oc.data_ptr(),
                                         cnt.data_ptr())

    def radius(r, nb, mc):
        return e.radius_outlier_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), n, r, nb, mc, (0.0, 0.0, 0.0), keep.data_ptr(),
                                       cnt.data_ptr(), pts.data_ptr(), oc.data_ptr(), idx.data_ptr())

    t_compute = [wall(compute)[0] for _ in range(2 + reps)][2:]
    got = [wall(compact) for _ in range(2 + reps)][2:]
    t_compact, n_valid = [g[0] for g in got], got[0][1]
    valid = torch.isfinite(dx).all(dim=2).flatten() & (df.flatten() > 0)
    n_ok = int(valid.sum())

    def mean_count(r):
        _, noor = radius(r, 1, FULL)
        return float(cnt.to(torch.int64).sum()) / max(n_ok - noor, 1), noor

    # radii by bisection on the mean of the full counts (it grows with the radius)
    z = dx[:, :, 2].flatten()
    zmed = float(z[valid].abs().median())
    radii = []
    for target in TARGETS:
        lo, hi = zmed * 1e-5, zmed * 0.02      # (the full count is quadratic in a large radius: the search stays below 2 % of the depth)
        for _ in range(30):
            mid = (lo * hi) ** 0.5
            got_mean, _ = mean_count(mid)
            lo, hi = (mid, hi) if got_mean < target else (lo, mid)
            if abs(got_mean - target) <= 0.03 * target:
                break
        radii.append((target, mid, got_mean))
    rec = dict(cloud=name, H=H, W=W, D=D, mode=mode, points=n, valid_points=n_ok, compute_ms=med(t_compute),
               compute_spread=spread(t_compute), compact_ms=med(t_compact), compact_spread=spread(t_compact), radius=[])
    for target, r, got_mean in radii:
        t_vox = [wall(lambda: voxel(r)) for _ in range(2 + reps)][2:]
        one = dict(target_mean_neighbours=target, radius=r, mean_neighbours=round(got_mean, 2), voxel_ms=med([g[0] for g in t_vox]),
                   voxel_spread=spread([g[0] for g in t_vox]), n_voxels=int(t_vox[0][1][0]), modes={})
        for label, nb, mc in MODES:
            t = {k: [] for k, _ in VARIANTS}
            nk = noor = 0
            for it in range(2 + reps):
                for which, bit in VARIANTS:   # alternating: all see the same minute
                    e.set_option(_lib.SGM_OPT_DEBUG, bit)
                    dt, (nk, noor) = wall(lambda: radius(r, nb, mc))
                    if it >= 2:
                        t[which].append(dt)
            stages = {}
            e.set_option(_lib.SGM_OPT_PROFILE, 1)
            for which, bit in VARIANTS:
                e.set_option(_lib.SGM_OPT_DEBUG, bit)
                runs = []
                for it in range(1 + reps):
                    radius(r, nb, mc)
                    runs.append({k: ms for k, ms, _ in e.stage_times() if k != "_wall"})
                stages[which] = {k: med([x[k] for x in runs[1:]]) for k in runs[0]}
            e.set_option(_lib.SGM_OPT_PROFILE, 0)
            e.set_option(_lib.SGM_OPT_DEBUG, 0)
            n_in = n_ok - noor
            cap = 1
            while cap < 2 * n_in:
                cap *= 2
            m = dict(nb_points=nb, max_count=mc, n_kept=int(nk), n_out_of_range=int(noor), points_in_range=int(n_in),
                     table_MB=round(cap * 16 / 2 ** 20, 1), ms={k: med(x) for k, x in t.items()}, spread={k: spread(x) for k, x in t.items()},
                     stages_ms=stages)
            m["over_compaction"] = round(m["ms"]["sorted"] / rec["compact_ms"], 2)
            m["over_voxel"] = round(m["ms"]["sorted"] / one["voxel_ms"], 2)
            m["query_over_compaction"] = round(stages["sorted"]["radius_query"] / rec["compact_ms"], 2)
            m["query_over_voxel"] = round(stages["sorted"]["radius_query"] / one["voxel_ms"], 2)
            m["share_of_compute"] = round(m["ms"]["sorted"] / rec["compute_ms"], 4)
            m["faster_order"] = "sorted" if m["ms"]["sorted"] <= m["ms"]["source"] else "source"
            one["modes"][label] = m
            print(json.dumps(dict(cloud=name, radius=r, mode=label, **{k: m[k] for k in ("ms", "stages_ms", "n_kept")})), flush=True)
        rec["radius"].append(one)
    results["clouds"].append(rec)
    print(json.dumps({k: x for k, x in rec.items() if k != "radius"}), flush=True)
    e.trim()
    del e, ta, tb, dd, df, dx, rgb, pts, oc, cnt, idx, keep
    torch.cuda.empty_cache()

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
