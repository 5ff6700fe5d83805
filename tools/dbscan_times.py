#!/usr/bin/env python3
"""What the density clustering costs, on the GPU box, in ONE run:

  for the device-resident XYZ image of a synthetic 4K D = 256 MODE_HH pair, and of a 1080p D = 128 and a 720p D = 64 pair
  (sgm_pipeline_device with the default Q), sgm_cluster_dbscan_device with every output at three eps found by bisection on the
  radius filter's counts so that the mean neighbour count of the points in range is about 4, 20 and 100, min_points 4 and 10;
  beside it, in the same run and alternating with it, the yardstick that walks the same candidates on the same grid:
  sgm_radius_outlier_device with the full count (max_count = 2^24 - 1); the A/B of the call: the core bit gathered by source index
  (SGM_DBG_DBSCAN_GATHER_CORE: `gather`) against the bit read with the sorted record (the default); and the case the call exists
  for: the centroids of sgm_voxel_downsample_device of each cloud (a voxel size that leaves a tenth of its valid points) as a point
  list, at an eps of twice the voxel size.

    tools/dbscan_times.py [reps [out.json]]        (default output: profiles/dbscan/times.json)

Times are host wall clock around blocking calls, two warm-up calls, median of `reps` with the spread, the variants alternating so
that all see the same minute; with SGM_OPT_PROFILE on in a second pass the stage record (HIP events) splits a call into
dbscan_count / dbscan_clear / dbscan_insert / dbscan_starts / dbscan_sort / dbscan_core / dbscan_link / dbscan_number /
dbscan_label.  `same_result` says that a variant returned the bytes of the default."""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "dbscan", "times.json")
SIZES = [("4K D256 HH", 2160, 3840, 256, 1), ("1080p D128 HH", 1080, 1920, 128, 1), ("720p D64 HH", 720, 1280, 64, 1)]
TARGETS = (4, 20, 100)
MIN_POINTS = (4, 10)
FULL = (1 << 24) - 1
GATHER = _lib.SGM_DBG_DBSCAN_GATHER_CORE
med = lambda v: round(statistics.median(v), 4)
spread = lambda v: [round(min(v), 4), round(max(v), 4)]
STATS = ("in_range", "out_of_range", "core", "border", "noise", "clusters")


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
    pts = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    lab = torch.empty(n, dtype=torch.int32, device="cuda")
    core = torch.empty(n, dtype=torch.uint8, device="cuda")
    sizes = torch.empty(n, dtype=torch.int32, device="cuda")
    cen = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    Q = synth.default_Q(W)

    def compute():
        e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, Q, dd.data_ptr(), df.data_ptr(), dx.data_ptr())
        e.synchronize()

    def radius(src, disp, m, r, nb=8, mc=FULL):
        return e.radius_outlier_device(src, disp, None, m, r, nb, mc, (0.0, 0.0, 0.0), keep.data_ptr(), cnt.data_ptr(), pts.data_ptr(),
                                       None, idx.data_ptr())

    def dbscan(src, disp, m, r, k, debug=0):
        e.set_option(_lib.SGM_OPT_DEBUG, debug)
        try:
            return e.cluster_dbscan_device(src, disp, m, r, k, (0.0, 0.0, 0.0), lab.data_ptr(), core.data_ptr(), sizes.data_ptr())
        finally:
            e.set_option(_lib.SGM_OPT_DEBUG, 0)

    def stages_of(fn):
        runs = []
        for it in range(1 + reps):
            fn()
            runs.append({k: ms for k, ms, _ in e.stage_times() if k != "_wall"})
        return {k: med([x[k] for x in runs[1:]]) for k in runs[0]}

    def measure(src, disp, m, r):
        """the calls at one eps on one cloud, alternating; the per-call record"""
        calls = [("radius_full", lambda: radius(src, disp, m, r))]
        for k in MIN_POINTS:
            calls.append((f"dbscan_k{k}", lambda k=k: dbscan(src, disp, m, r, k)))
            calls.append((f"dbscan_k{k}_gather", lambda k=k: dbscan(src, disp, m, r, k, GATHER)))
        t = {label: [] for label, _ in calls}
        out_bytes = {}
        for it in range(2 + reps):
            for label, fn in calls:
                dt, res = wall(fn)
                if it >= 2:
                    t[label].append(dt)
                if it == 0 and label.startswith("dbscan"):
                    nc, st = res
                    out_bytes[label] = (lab[:m].cpu().numpy().tobytes(), core[:m].cpu().numpy().tobytes(), sizes[:nc].cpu().numpy().tobytes(),
                                        st.tolist())
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        stages = {label: stages_of(fn) for label, fn in calls}
        e.set_option(_lib.SGM_OPT_PROFILE, 0)
        rq = stages["radius_full"]["radius_query"]
        one = dict(eps=r, radius_full=dict(ms=med(t["radius_full"]), spread=spread(t["radius_full"]), stages_ms=stages["radius_full"]))
        for k in MIN_POINTS:
            label = f"dbscan_k{k}"
            s, g = stages[label], stages[label + "_gather"]
            one[label] = dict(ms=med(t[label]), spread=spread(t[label]), stages_ms=s, stats=dict(zip(STATS, out_bytes[label][3])),
                              call_over_radius_full=round(med(t[label]) / med(t["radius_full"]), 2),
                              link_over_radius_query=round(s["dbscan_link"] / rq, 2), core_over_radius_query=round(s["dbscan_core"] / rq, 2))
            one[label + "_gather"] = dict(ms=med(t[label + "_gather"]), spread=spread(t[label + "_gather"]), stages_ms=g,
                                          same_result=out_bytes[label + "_gather"] == out_bytes[label],
                                          link_over_default_link=round(g["dbscan_link"] / s["dbscan_link"], 3))
        return one

    t_compute = [wall(compute)[0] for _ in range(2 + reps)][2:]
    valid = torch.isfinite(dx).all(dim=2).flatten() & (df.flatten() > 0)
    n_ok = int(valid.sum())

    def mean_count(src, disp, m, m_ok, r):
        _, noor = radius(src, disp, m, r, 1, FULL)
        return float(cnt[:m].to(torch.int64).sum()) / max(m_ok - noor, 1)

    z = dx[:, :, 2].flatten()
    zmed = float(z[valid].abs().median())
    rec = dict(cloud=name, H=H, W=W, D=D, mode=mode, points=n, valid_points=n_ok, compute_ms=med(t_compute),
               compute_spread=spread(t_compute), eps=[])
    for target in TARGETS:      # eps by bisection on the mean of the full counts, as tools/radius_times.py finds its radii
        lo, hi = zmed * 1e-5, zmed * 0.02
        for _ in range(30):
            r = (lo * hi) ** 0.5
            got_mean = mean_count(dx.data_ptr(), df.data_ptr(), n, n_ok, r)
            lo, hi = (r, hi) if got_mean < target else (lo, r)
            if abs(got_mean - target) <= 0.03 * target:
                break
        one = dict(target_mean_neighbours=target, mean_neighbours=round(got_mean, 2), **measure(dx.data_ptr(), df.data_ptr(), n, r))
        for k in MIN_POINTS:
            one[f"dbscan_k{k}"]["share_of_compute"] = round(one[f"dbscan_k{k}"]["ms"] / rec["compute_ms"], 4)
        print(json.dumps(dict(cloud=name, **one)), flush=True)
        rec["eps"].append(one)
    # the centroids of the voxel grid as a point list: a voxel size (bisection) that leaves about a tenth of the valid points
    want = max(n_ok // 10, 1000)
    lo, hi = zmed * 1e-5, zmed * 0.05
    for _ in range(30):
        voxel = (lo * hi) ** 0.5
        nv, _ = e.voxel_downsample_device(dx.data_ptr(), df.data_ptr(), None, n, voxel, (0.0, 0.0, 0.0), 1, cen.data_ptr())
        lo, hi = (lo, voxel) if nv < want else (voxel, hi)
        if abs(nv - want) <= 0.05 * want:
            break
    r = 2 * voxel
    got_mean = mean_count(cen.data_ptr(), None, nv, nv, r)
    rec["centroids"] = dict(voxel_size=voxel, points=int(nv), mean_neighbours=round(got_mean, 2), **measure(cen.data_ptr(), None, int(nv), r))
    for k in MIN_POINTS:
        rec["centroids"][f"dbscan_k{k}"]["share_of_compute"] = round(rec["centroids"][f"dbscan_k{k}"]["ms"] / rec["compute_ms"], 4)
    print(json.dumps(dict(cloud=name, centroids=rec["centroids"])), flush=True)
    results["clouds"].append(rec)
    e.trim()
    del e, ta, tb, dd, df, dx, pts, cnt, idx, keep, lab, core, sizes, cen
    torch.cuda.empty_cache()

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
