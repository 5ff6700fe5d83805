#!/usr/bin/env python3
"""What the plane segmentation costs, on the GPU box, in ONE run:

  for the device-resident XYZ image of a synthetic 4K D = 256 MODE_HH pair, and of a 1080p D = 128 and a 720p D = 64 pair
  (sgm_pipeline_device with the default Q), sgm_segment_plane_device with every output at K = 100, 1000 and 4096 hypotheses under
  both forms of the counting kernel -- the default and SGM_DBG_PLANE_OTHER_COUNT (`other`), alternating --; sgm_plane_inliers_device
  alone on the model found; and beside them, in the same run, the two yardsticks the README measures the call against:
  sgm_compact_points_device, which reads the cloud once, and sgm_radius_outlier_device with the full count (max_count = 2^24 - 1) at
  a radius found by bisection so that the mean neighbour count of the points in range is about 20.

    tools/plane_times.py [reps [out.json]]        (default output: profiles/plane/times.json)

Times are host wall clock around blocking calls, two warm-up calls, median of `reps` with the spread (min, max), the variants
alternating so that all see the same minute; with SGM_OPT_PROFILE on in a second pass the stage record (HIP events) splits a call
into plane_valid / plane_sample / plane_count / plane_best / plane_moments / plane_solve / plane_classify / plane_compact, and
`pairs_per_ns` is valid points x K over the plane_count stage.  `same_result` says that the other form returned the bytes of the
default.  `which_is_default` names the form that ran without the debug bit (kernels_plane.h: PLANE_DEFAULT_MFMA)."""
import json
import os
import re
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

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "plane", "times.json")
SIZES = [("4K D256 HH", 2160, 3840, 256, 1), ("1080p D128 HH", 1080, 1920, 128, 1), ("720p D64 HH", 720, 1280, 64, 1)]
KS = (100, 1000, 4096)
FULL = (1 << 24) - 1
OTHER = _lib.SGM_DBG_PLANE_OTHER_COUNT
med = lambda v: round(statistics.median(v), 4)
spread = lambda v: [round(min(v), 4), round(max(v), 4)]
STATS = cv.pointcloud.PLANE_STATS
src = open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "kernels_plane.h")).read()
default_form = "mfma" if re.search(r"PLANE_DEFAULT_MFMA = true", src) else "valu"
other_form = "valu" if default_form == "mfma" else "mfma"


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


results = dict(reps=reps, which_is_default=default_form, other=other_form, clouds=[])
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
    inl = torch.empty(n, dtype=torch.uint8, device="cuda")
    dist = torch.empty(n, dtype=torch.float32, device="cuda")
    Q = synth.default_Q(W)

    def compute():
        e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, Q, dd.data_ptr(), df.data_ptr(), dx.data_ptr())
        e.synchronize()

    def radius(r, nb=8, mc=FULL):
        return e.radius_outlier_device(dx.data_ptr(), df.data_ptr(), None, n, r, nb, mc, (0.0, 0.0, 0.0), keep.data_ptr(), cnt.data_ptr(),
                                       pts.data_ptr(), None, idx.data_ptr())

    def compact():
        return e.compact_points_device(dx.data_ptr(), df.data_ptr(), None, n, pts.data_ptr(), None)

    def plane(K, debug=0, refine=True):
        e.set_option(_lib.SGM_OPT_DEBUG, debug)
        try:
            return e.segment_plane_device(dx.data_ptr(), df.data_ptr(), None, n, thr, K, 1, refine, 0, inl.data_ptr(), dist.data_ptr(),
                                          pts.data_ptr(), None, idx.data_ptr())
        finally:
            e.set_option(_lib.SGM_OPT_DEBUG, 0)

    def inliers(model):
        return e.plane_inliers_device(dx.data_ptr(), df.data_ptr(), None, n, model, thr, 0, inl.data_ptr(), dist.data_ptr(), pts.data_ptr(), None,
                                      idx.data_ptr())

    def stages_of(fn):
        runs = []
        for it in range(1 + reps):
            fn()
            runs.append({k: ms for k, ms, _ in e.stage_times() if k != "_wall"})
        return {k: med([x[k] for x in runs[1:]]) for k in runs[0]}

    t_compute = [wall(compute)[0] for _ in range(2 + reps)][2:]
    valid = torch.isfinite(dx).all(dim=2).flatten() & (df.flatten() > 0)
    n_ok = int(valid.sum())
    zmed = float(dx[:, :, 2].flatten()[valid].abs().median())
    thr = float(torch.tensor(zmed * 0.01, dtype=torch.float32))
    # the radius filter's radius: bisection on the mean of the full counts, as tools/radius_times.py finds its radii
    lo, hi = zmed * 1e-5, zmed * 0.02
    for _ in range(30):
        r = (lo * hi) ** 0.5
        _, noor = radius(r, 1, FULL)
        got_mean = float(cnt.to(torch.int64).sum()) / max(n_ok - noor, 1)
        lo, hi = (r, hi) if got_mean < 20 else (lo, r)
        if abs(got_mean - 20) <= 0.6:
            break
    model0 = plane(1000)[0]
    calls = [("compact_points", compact), ("radius_full", lambda: radius(r)), ("plane_inliers", lambda: inliers(model0))]
    for K in KS:
        calls.append((f"plane_K{K}", lambda K=K: plane(K)))
        calls.append((f"plane_K{K}_other", lambda K=K: plane(K, OTHER)))
    t = {label: [] for label, _ in calls}
    out_bytes = {}
    for it in range(2 + reps):
        for label, fn in calls:
            dt, res = wall(fn)
            if it >= 2:
                t[label].append(dt)
            if it == 0 and label.startswith("plane_K"):
                model, st, ni, ns = res
                out_bytes[label] = (model.tobytes(), st.tolist(), ni, ns, inl.cpu().numpy().tobytes(), dist.cpu().numpy().tobytes(),
                                    idx[:ns].cpu().numpy().tobytes())
    e.set_option(_lib.SGM_OPT_PROFILE, 1)
    stages = {label: stages_of(fn) for label, fn in calls if label != "compact_points"}      # (the compaction keeps no stage record)
    e.set_option(_lib.SGM_OPT_PROFILE, 0)
    rec = dict(cloud=name, H=H, W=W, D=D, mode=mode, points=n, valid_points=n_ok, compute_ms=med(t_compute), compute_spread=spread(t_compute),
               distance_threshold=thr, radius=r, radius_mean_neighbours=round(got_mean, 2))
    for label in ("compact_points", "radius_full", "plane_inliers"):
        rec[label] = dict(ms=med(t[label]), spread=spread(t[label]), stages_ms=stages.get(label))
    for K in KS:
        label = f"plane_K{K}"
        for lab, form in ((label, default_form), (label + "_other", other_form)):
            s = stages[lab]
            rec[lab] = dict(form=form, ms=med(t[lab]), spread=spread(t[lab]), stages_ms=s, stats=dict(zip(STATS, out_bytes[lab][1])),
                            model=np.frombuffer(out_bytes[lab][0], np.float32).tolist(),
                            pairs_per_ns=round(n_ok * K / (s["plane_count"] * 1e6), 2),
                            call_over_compact=round(med(t[lab]) / med(t["compact_points"]), 2),
                            call_over_radius_full=round(med(t[lab]) / med(t["radius_full"]), 3),
                            share_of_compute=round(med(t[lab]) / med(t_compute), 4))
        rec[label + "_other"]["same_result"] = out_bytes[label + "_other"] == out_bytes[label]
        rec[label + "_other"]["count_over_default_count"] = round(stages[label + "_other"]["plane_count"] / stages[label]["plane_count"], 3)
    print(json.dumps(rec), flush=True)
    results["clouds"].append(rec)
    e.trim()
    del e, ta, tb, dd, df, dx, pts, cnt, idx, keep, inl, dist
    torch.cuda.empty_cache()

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
