#!/usr/bin/env python3
"""What the statistical outlier removal costs, on the GPU box, in ONE run:

  for the device-resident XYZ image of a synthetic 4K D = 256 MODE_HH pair, and of a 1080p D = 128 and a 720p D = 64 pair
  (sgm_pipeline_device with the default Q), sgm_statistical_outlier_device with every output at two values of max_radius found
  by bisection on the radius filter's counts so that the mean neighbour count of the points in range is about 20 and 100 -- each
  with nb_neighbors = 8, 20 and 64 (one instance of k_stat_query per list capacity 8, 32 and 64) and std_ratio = 1; beside them,
  in the same run and alternating with them, the yardstick: sgm_radius_outlier_device at the same radius with the full count
  (max_count = 2^24 - 1), which walks the same candidates and has nothing to select; nb_neighbors = 8 and 20 once more with
  the 64-word list (SGM_DBG_STAT_WIDE_LIST: `k8_wide`, `k20_wide`), which separates what the list's capacity costs from what k
  costs; and the pair's own compute.

    tools/statistical_times.py [reps [out.json]]        (default output: profiles/statistical/times.json)

Times are host wall clock around calls that end in a synchronise (the entries block for their counts), two warm-up calls, median
of `reps` with the spread; with SGM_OPT_PROFILE on in a second pass the stage record (HIP events) splits a call into stat_count /
stat_clear / stat_insert / stat_starts / stat_sort / stat_query / stat_reduce / stat_keep / stat_compact.  `radius_then` is what
profiles/radius/times.json holds for the yardstick at the same target (full_count, sorted), from the run that file was written by:
the two agree within the run-to-run spread if factoring the grid build out of the radius entry moved nothing."""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "statistical", "times.json")
SIZES = [("4K D256 HH", 2160, 3840, 256, 1), ("1080p D128 HH", 1080, 1920, 128, 1), ("720p D64 HH", 720, 1280, 64, 1)]
TARGETS = (20, 100)
KS = (8, 20, 64)
FULL = (1 << 24) - 1
WIDE = _lib.SGM_DBG_STAT_WIDE_LIST
med = lambda v: round(statistics.median(v), 4)
spread = lambda v: [round(min(v), 4), round(max(v), 4)]

then = {}
try:
    with open(os.path.join(ROOT, "profiles", "radius", "times.json")) as f:
        for c in json.load(f)["clouds"]:
            for one in c["radius"]:
                m = one["modes"]["full_count"]
                then[(c["cloud"], one["target_mean_neighbours"])] = dict(radius=one["radius"], ms=m["ms"]["sorted"], spread=m["spread"]["sorted"],
                                                                         stages_ms=m["stages_ms"]["sorted"])
except OSError:
    pass


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


results = dict(reps=reps, clouds=[])
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
    mean = torch.empty(n, dtype=torch.float32, device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    Q = synth.default_Q(W)

    def compute():
        e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, Q, dd.data_ptr(), df.data_ptr(), dx.data_ptr())
        e.synchronize()

    def radius(r, nb=8, mc=FULL):
        return e.radius_outlier_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), n, r, nb, mc, (0.0, 0.0, 0.0), keep.data_ptr(),
                                       cnt.data_ptr(), pts.data_ptr(), oc.data_ptr(), idx.data_ptr())

    def statistical(r, k):
        return e.statistical_outlier_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), n, k, 1.0, r, (0.0, 0.0, 0.0), keep.data_ptr(),
                                            mean.data_ptr(), pts.data_ptr(), oc.data_ptr(), idx.data_ptr())

    def stages_of(fn):
        runs = []
        for it in range(1 + reps):
            fn()
            runs.append({k: ms for k, ms, _ in e.stage_times() if k != "_wall"})
        return {k: med([x[k] for x in runs[1:]]) for k in runs[0]}

    t_compute = [wall(compute)[0] for _ in range(2 + reps)][2:]
    valid = torch.isfinite(dx).all(dim=2).flatten() & (df.flatten() > 0)
    n_ok = int(valid.sum())

    def mean_count(r):
        _, noor = radius(r, 1, FULL)
        return float(cnt.to(torch.int64).sum()) / max(n_ok - noor, 1), noor

    # radii by bisection on the mean of the full counts (it grows with the radius), as tools/radius_times.py finds them
    z = dx[:, :, 2].flatten()
    zmed = float(z[valid].abs().median())
    rec = dict(cloud=name, H=H, W=W, D=D, mode=mode, points=n, valid_points=n_ok, compute_ms=med(t_compute),
               compute_spread=spread(t_compute), radius=[])
    for target in TARGETS:
        lo, hi = zmed * 1e-5, zmed * 0.02
        for _ in range(30):
            r = (lo * hi) ** 0.5
            got_mean, _ = mean_count(r)
            lo, hi = (r, hi) if got_mean < target else (lo, r)
            if abs(got_mean - target) <= 0.03 * target:
                break
        def wide(k_):
            e.set_option(_lib.SGM_OPT_DEBUG, WIDE)
            try:
                return statistical(r, k_)
            finally:
                e.set_option(_lib.SGM_OPT_DEBUG, 0)
        calls = ([("radius_full", lambda: radius(r))] + [(f"k{k}", (lambda k_: lambda: statistical(r, k_))(k)) for k in KS]
                 + [(f"k{k}_wide", (lambda k_: lambda: wide(k_))(k)) for k in KS[:2]])
        t = {label: [] for label, _ in calls}
        last = {}
        for it in range(2 + reps):
            for label, fn in calls:       # alternating: all see the same minute
                dt, last[label] = wall(fn)
                if it >= 2:
                    t[label].append(dt)
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        stages = {label: stages_of(fn) for label, fn in calls}
        e.set_option(_lib.SGM_OPT_PROFILE, 0)
        yard_ms, yard_q = med(t["radius_full"]), stages["radius_full"]["radius_query"]
        one = dict(target_mean_neighbours=target, max_radius=r, mean_neighbours=round(got_mean, 2),
                   wide_list={f"{k}": dict(ms=med(t[f"k{k}_wide"]), spread=spread(t[f"k{k}_wide"]), stat_query_ms=stages[f"k{k}_wide"]["stat_query"],
                                           same_result=bool(last[f"k{k}_wide"][0] == last[f"k{k}"][0] and (last[f"k{k}_wide"][1] == last[f"k{k}"][1]).all()))
                              for k in KS[:2]},
                   radius_full=dict(ms=yard_ms, spread=spread(t["radius_full"]), stages_ms=stages["radius_full"], n_kept=int(last["radius_full"][0]),
                                    radius_then=then.get((name, target))), k={})
        for k in KS:
            label = f"k{k}"
            nk, st = last[label]
            ms = med(t[label])
            one["k"][str(k)] = dict(ms=ms, spread=spread(t[label]), stages_ms=stages[label], n_kept=int(nk),
                                    stats=dict(zip(("in_range", "out_of_range", "dense", "sparse", "A", "B", "T"), (int(x) for x in st[:7]))),
                                    call_over_radius_full=round(ms / yard_ms, 2),
                                    query_over_radius_query=round(stages[label]["stat_query"] / yard_q, 2),
                                    share_of_compute=round(ms / rec["compute_ms"], 4))
            print(json.dumps(dict(cloud=name, max_radius=r, k=k, **one["k"][str(k)])), flush=True)
        print(json.dumps(dict(cloud=name, max_radius=r, wide_list=one["wide_list"], **one["radius_full"])), flush=True)
        rec["radius"].append(one)
    results["clouds"].append(rec)
    e.trim()
    del e, ta, tb, dd, df, dx, rgb, pts, oc, cnt, mean, idx, keep
    torch.cuda.empty_cache()

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
