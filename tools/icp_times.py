#!/usr/bin/env python3
"""What the rigid registration costs, on the GPU box, in ONE run:

  for the device-resident XYZ image of a synthetic 4K D = 256 MODE_HH pair, and of a 1080p D = 128 and a 720p D = 64 pair
  (sgm_pipeline_device with the default Q), against a copy of it moved by a known motion (sgm_transform_points_device), and for the
  voxel centroids of both (sgm_voxel_downsample_device, voxel = the radius below) registered at twice the voxel size: one
  evaluation (sgm_evaluate_registration_device; sgm_register_icp_device with max_iteration = 0 under point-to-plane), the per-stage
  split of it, and a 30-iteration call with both thresholds 0 under both estimations; and beside them, in the same run, the
  yardstick every consumer of the grid is held against: sgm_radius_outlier_device with the full count (max_count = 2^24 - 1) at the
  SAME radius on the target cloud.  The radius of the full cloud is found by bisection so that the mean neighbour count of the
  points in range is about 20.

    tools/icp_times.py [reps [out.json]]        (default output: profiles/icp/times.json)

Times are host wall clock around blocking calls, two warm-up calls, median of `reps` with the spread (min, max), the calls
alternating so that all see the same minute; with SGM_OPT_PROFILE on in a second pass the stage record (HIP events) splits a call
into icp_count .. icp_sort (the target's grid) and icp_correspond / icp_terms / icp_reduce (the last evaluation).
`correspond_over_radius_query` is the correspondence stage as a multiple of the radius filter's query stage."""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "icp", "times.json")
SIZES = [("4K D256 HH", 2160, 3840, 256, 1), ("1080p D128 HH", 1080, 1920, 128, 1), ("720p D64 HH", 720, 1280, 64, 1)]
FULL = (1 << 24) - 1
med = lambda v: round(statistics.median(v), 4)
spread = lambda v: [round(min(v), 4), round(max(v), 4)]
STATS = cv.pointcloud.ICP_STATS


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def motion(r, depth):
    """a rotation about an oblique axis that moves a point at the median depth by 0.3 r, and a translation of about half of r"""
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    th = 0.3 * r / depth
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = np.array([0.3, -0.3, 0.25]) * r
    return T


results = dict(reps=reps, clouds=[])
for name, H, W, D, mode in SIZES:
    a, b = synth.make_pair(H, W, D, 1234)[:2]
    e = cv.Engine(bench.sgbm_params(D, 7, mode))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    n = H * W
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
    dd = torch.empty((H, W), dtype=torch.int16, device="cuda")
    df, dx, dx2, nrm = f32(H, W), f32(H, W, 3), f32(H, W, 3), f32(n, 3)
    corr, d2, cnt = i32(n), f32(n), i32(n)
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    vs, vt, vn = f32(n, 3), f32(n, 3), f32(n, 3)
    Q = synth.default_Q(W)
    e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, Q, dd.data_ptr(), df.data_ptr(), dx.data_ptr())
    e.synchronize()

    def radius(xyz, disp, m, r, nb=8, mc=FULL):
        return e.radius_outlier_device(xyz.data_ptr(), None if disp is None else disp.data_ptr(), None, m, r, nb, mc, (0.0, 0.0, 0.0),
                                       keep.data_ptr(), cnt.data_ptr(), None, None, None)

    valid = torch.isfinite(dx).all(dim=2).flatten() & (df.flatten() > 0)
    n_ok = int(valid.sum())
    zmed = float(dx[:, :, 2].flatten()[valid].abs().median())
    lo, hi = zmed * 1e-5, zmed * 0.02
    for _ in range(30):      # the radius: bisection on the mean of the full counts, as tools/radius_times.py finds its radii
        r = (lo * hi) ** 0.5
        _, noor = radius(dx, df, n, r, 1, FULL)
        got_mean = float(cnt[:n].to(torch.int64).sum()) / max(n_ok - noor, 1)
        lo, hi = (r, hi) if got_mean < 20 else (lo, r)
        if abs(got_mean - 20) <= 0.6:
            break
    r = float(np.float32(r))
    truth = motion(r, zmed)
    e.transform_points_device(dx.data_ptr(), None, n, truth, dx2.data_ptr())
    e.synchronize()
    # the voxel centroids of both clouds, voxel = r, registered at 2 r
    ms, _ = e.voxel_downsample_device(dx.data_ptr(), df.data_ptr(), None, n, r, (0.0, 0.0, 0.0), 1, vs.data_ptr())
    mt, _ = e.voxel_downsample_device(dx2.data_ptr(), df.data_ptr(), None, n, r, (0.0, 0.0, 0.0), 1, vt.data_ptr())
    e.covariance_normals_device(vt.data_ptr(), None, mt, 2 * r, 3, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), True, vn.data_ptr())
    e.covariance_normals_device(dx2.data_ptr(), df.data_ptr(), n, r, 3, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), True, nrm.data_ptr())
    rec = dict(cloud=name, H=H, W=W, D=D, points=n, valid_points=n_ok, radius=r, radius_mean_neighbours=round(got_mean, 2),
               centroids_source=ms, centroids_target=mt, true_motion=truth.tolist())
    for label, S, DS, NS, Tg, DT, N, NT, rr in (("full", dx, df, n, dx2, df, nrm, n, r), ("centroids", vs, None, ms, vt, None, vn, mt, 2 * r)):
        ptr = lambda t: None if t is None else t.data_ptr()

        def evaluate():
            return e.evaluate_registration_device(S.data_ptr(), ptr(DS), NS, Tg.data_ptr(), ptr(DT), NT, rr, (0.0, 0.0, 0.0), None,
                                                  corr.data_ptr(), d2.data_ptr())

        def register(est, maxit):
            return e.register_icp_device(S.data_ptr(), ptr(DS), NS, Tg.data_ptr(), ptr(DT), N.data_ptr(), NT, rr, (0.0, 0.0, 0.0), None, est,
                                         maxit, 0.0, 0.0, corr.data_ptr(), d2.data_ptr())

        calls = [("radius_full", lambda: radius(Tg, DT, NT, rr)), ("evaluate", evaluate), ("plane_0_iterations", lambda: register(1, 0)),
                 ("point_30_iterations", lambda: register(0, 30)), ("plane_30_iterations", lambda: register(1, 30))]
        t = {k: [] for k, _ in calls}
        last = {}
        for it in range(2 + reps):
            for k, fn in calls:
                dt, res = wall(fn)
                last[k] = res
                if it >= 2:
                    t[k].append(dt)
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        stages = {}
        for k, fn in calls:
            runs = []
            for it in range(1 + reps):
                fn()
                runs.append({s: ms_ for s, ms_, _ in e.stage_times() if s != "_wall"})
            stages[k] = {s: med([x[s] for x in runs[1:]]) for s in runs[0]}
        e.set_option(_lib.SGM_OPT_PROFILE, 0)
        out = dict(source_points=NS, target_points=NT, max_correspondence_distance=rr)
        for k, _ in calls:
            out[k] = dict(ms=med(t[k]), spread=spread(t[k]), stages_ms=stages[k])
        out["evaluate"].update(fitness=last["evaluate"][0], rmse=last["evaluate"][1], stats=dict(zip(STATS, (int(x) for x in last["evaluate"][2]))))
        for k in ("point_30_iterations", "plane_30_iterations"):
            T, fit, rmse, hist, st = last[k]
            E = T @ np.linalg.inv(truth)
            out[k].update(fitness=fit, rmse=rmse, stats=dict(zip(STATS, (int(x) for x in st))), T=T.tolist(),
                          rotation_error=float(np.linalg.norm([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]) / 2),
                          translation_error_over_r=float(np.linalg.norm(T[:3, 3] - truth[:3, 3]) / rr),
                          ms_per_iteration=round(med(t[k]) / max(int(st[3]), 1), 4))
        ev = stages["evaluate"]
        out["correspond_over_radius_query"] = round(ev["icp_correspond"] / stages["radius_full"]["radius_query"], 3)
        out["evaluate_over_radius_full"] = round(med(t["evaluate"]) / med(t["radius_full"]), 3)
        out["terms_and_reduce_over_correspond"] = round((ev["icp_terms"] + ev["icp_reduce"]) / ev["icp_correspond"], 3)
        rec[label] = out
    print(json.dumps(rec), flush=True)
    results["clouds"].append(rec)
    e.trim()
    del e, ta, tb, dd, df, dx, dx2, nrm, corr, d2, cnt, keep, vs, vt, vn
    torch.cuda.empty_cache()

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
