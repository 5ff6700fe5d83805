#!/usr/bin/env python3
"""What the signed distance volume costs, on the GPU box, in ONE run:

  for the device-resident XYZ image of a synthetic 4K D = 256 MODE_HH pair, and of a 1080p D = 128 and a 720p D = 64 pair
  (sgm_pipeline_device with the default Q), one frame integrated into a 512^3 and a 256^3 volume sized to the scene (the box of the
  5th to 95th percentile of the valid points, voxel = its longest side / n, trunc = 4 voxels), with and without colour sums, and
  the extraction of the crossings from the volume as the timed integrations of that one frame left it (every seen voxel then has
  the same weight, which is the call's min_weight); the integration once more with the eight counts asked for
  (six ballots, one atomic instruction of up to six lanes per wave, the second launch and the wait); the same volume moved sideways out
  of the frustum, where every voxel is outside; and beside them, in the same run, the two yardsticks:
  a plain device copy of the same planes (torch), and sgm_compact_points_device on the frame's cloud.

    tools/tsdf_times.py [reps [out.json]]        (default output: profiles/tsdf/times.json)

Times: the stage record (HIP events around each stage, SGM_OPT_PROFILE) and the host wall clock around the blocking call, two warm-up
calls, median of `reps` with the spread.  Bytes: `plane_bytes` is what the definition makes a kernel move in the planes, computed from
the call's own counts -- integration: 4 per voxel that reaches step 7 (its weight) + 12 per updated voxel (sum read and written,
weight written) + 24 per updated voxel with colour; count: 4 V (every weight) + 4 per voxel with weight >= min_weight (its sum), the
neighbours counted as cache hits; emit: the same for the blocks that hold a crossing, + 12 (15 with colour) per row written.
`dense_bytes` is the same plane set read and written once in full (what the copy moves).  The brick-level early-out is not built:
`all_outside_stage_ms` against `stage_ms`, with the share of outside voxels in `stats`, bounds what it could save."""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "tsdf", "times.json")
SIZES = [("4K D256 HH", 2160, 3840, 256, 1), ("1080p D128 HH", 1080, 1920, 128, 1), ("720p D64 HH", 720, 1280, 64, 1)]
med = lambda v: round(statistics.median(v), 4)
spread = lambda v: [round(min(v), 4), round(max(v), 4)]
gbps = lambda b, ms: round(b / ms / 1e6, 1) if ms > 0 else None
STATS = cv.pointcloud.TSDF_STATS


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


results = dict(reps=reps, brick_early_out="not built", frames=[])
for name, H, W, D, mode in SIZES:
    a, b = synth.make_pair(H, W, D, 1234)[:2]
    e = cv.Engine(bench.sgbm_params(D, 7, mode))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    n = H * W
    dd = torch.empty((H, W), dtype=torch.int16, device="cuda")
    df = torch.empty((H, W), dtype=torch.float32, device="cuda")
    dx = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    col = torch.from_numpy(np.repeat(a[..., None], 3, axis=2).copy()).cuda()
    Q = synth.default_Q(W)
    e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, Q, dd.data_ptr(), df.data_ptr(), dx.data_ptr())
    e.synchronize()
    cam, front = cv.camera_from_Q(Q)
    valid = torch.isfinite(dx).all(dim=2) & (df > 0)
    pts = dx[valid].cpu().numpy()
    lo, hi = np.percentile(pts, 5, axis=0), np.percentile(pts, 95, axis=0)
    rec = dict(frame=name, H=H, W=W, D=D, pixels=n, valid_pixels=int(valid.sum()), volumes=[])
    # the yardstick of every cloud call: the ordered compaction of the frame's cloud
    cp, cc = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    t = []
    for it in range(2 + reps):
        dt, nv = wall(lambda: e.compact_points_device(dx.data_ptr(), df.data_ptr(), col.data_ptr(), n, cp.data_ptr(), cc.data_ptr()))
        if it >= 2:
            t.append(dt)
    rec["compact_points_device"] = dict(ms=med(t), spread=spread(t), valid=int(nv))
    del cp, cc
    for nvox in (512, 256):
        dims = (nvox, nvox, nvox)
        V = nvox ** 3
        vs = float(np.float32(max(hi - lo) / nvox))
        origin = (0.5 * (lo + hi) - 0.5 * nvox * vs).astype(np.float32)
        tau = float(np.float32(4 * vs))
        for color in (True, False):
            s = torch.zeros(V, dtype=torch.int32, device="cuda")
            w = torch.zeros(V, dtype=torch.int32, device="cuda")
            rgb = torch.zeros(3 * V, dtype=torch.int32, device="cuda") if color else None
            rp = None if rgb is None else rgb.data_ptr()
            cptr = col.data_ptr() if color else None

            def integrate(stats):
                return e.tsdf_integrate_device(dims, vs, tau, origin, s.data_ptr(), w.data_ptr(), rp, dx.data_ptr(), df.data_ptr(), cptr, H, W, cam,
                                               front, np.eye(4), stats=stats)
            out = dict(dims=dims, voxel_size=vs, sdf_trunc=tau, color=color, voxels=V, dense_bytes=2 * V * (20 if color else 8))
            st = integrate(True)
            out["stats"] = dict(zip(STATS, (int(x) for x in st[:7])))
            upd, sat = int(st[0]), int(st[4])
            out["integrate_plane_bytes"] = pb = 4 * (upd + sat) + 12 * upd + (24 * upd if color else 0)
            tw, ts_ = [], []
            for it in range(2 + reps):
                dt, _ = wall(lambda: integrate(False))
                if it >= 2:
                    tw.append(dt)
            tws = []
            for it in range(2 + reps):
                dt, _ = wall(lambda: integrate(True))
                if it >= 2:
                    tws.append(dt)
            e.set_option(_lib.SGM_OPT_PROFILE, 1)
            tss = []
            for it in range(1 + reps):
                integrate(False)
                ms = dict((k, v) for k, v, _ in e.stage_times())["tsdf_integrate"]
                integrate(True)
                ms_s = dict((k, v) for k, v, _ in e.stage_times())["tsdf_integrate"]
                if it >= 1:
                    ts_.append(ms)
                    tss.append(ms_s)
            # the same volume moved out of the frustum: every voxel is outside after steps 1 to 4 and touches no plane -- what the
            # arithmetic alone costs, and the most a brick-level early-out could save on this share of a volume
            far = origin + np.array([1e4 * nvox * vs, 0, 0], np.float32)      # (sideways: still in front, so step 4 runs)
            t_out = []
            for it in range(1 + reps):
                st_far = e.tsdf_integrate_device(dims, vs, tau, far, s.data_ptr(), w.data_ptr(), rp, dx.data_ptr(), df.data_ptr(), cptr, H, W, cam,
                                                 front, np.eye(4), stats=(it == 0))
                e.synchronize()
                if it == 0:
                    assert int(st_far[5]) == V, st_far
                else:
                    t_out.append(dict((k, v) for k, v, _ in e.stage_times())["tsdf_integrate"])
            e.set_option(_lib.SGM_OPT_PROFILE, 0)
            out["integrate"] = dict(wall_ms=med(tw), wall_spread=spread(tw), stage_ms=med(ts_), stage_spread=spread(ts_),
                                    plane_GBps=gbps(pb, med(ts_)), dense_equivalent_GBps=gbps(out["dense_bytes"], med(ts_)),
                                    with_counts_stage_ms=med(tss), with_counts_spread=spread(tss), with_counts_wall_ms=med(tws),
                                    all_outside_stage_ms=med(t_out), all_outside_spread=spread(t_out))
            # the plain copy of the same planes, in the same minute (torch events)
            planes = [x for x in (s, w, rgb) if x is not None]
            dst = [torch.empty_like(x) for x in planes]
            tc = []
            for it in range(2 + reps):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for x, y in zip(planes, dst):
                    y.copy_(x)
                ev1.record()
                torch.cuda.synchronize()
                if it >= 2:
                    tc.append(ev0.elapsed_time(ev1))
            out["plane_copy"] = dict(ms=med(tc), spread=spread(tc), GBps=gbps(out["dense_bytes"], med(tc)))
            del dst
            # the extraction, from the volume as the integrations above left it (every seen voxel has the same weight)
            mw = int(w.max())
            seen = int((w >= mw).sum())
            total = e.tsdf_extract_device(dims, vs, origin, s.data_ptr(), w.data_ptr(), rp, mw)
            op = torch.empty((total, 3), dtype=torch.float32, device="cuda")
            oc = torch.empty((total, 3), dtype=torch.uint8, device="cuda") if color else None

            def extract():
                return e.tsdf_extract_device(dims, vs, origin, s.data_ptr(), w.data_ptr(), rp, mw, total, op.data_ptr(),
                                             None if oc is None else oc.data_ptr())
            tw = []
            for it in range(2 + reps):
                dt, got = wall(extract)
                assert got == total
                if it >= 2:
                    tw.append(dt)
            e.set_option(_lib.SGM_OPT_PROFILE, 1)
            runs = []
            for it in range(1 + reps):
                extract()
                runs.append({k: v for k, v, _ in e.stage_times() if k != "_wall"})
            e.set_option(_lib.SGM_OPT_PROFILE, 0)
            stages = {k: med([r[k] for r in runs[1:]]) for k in runs[0]}
            cb = 4 * V + 4 * seen
            eb = cb + total * (15 if color else 12)
            out["extract"] = dict(min_weight=mw, seen_voxels=seen, crossings=int(total), wall_ms=med(tw), wall_spread=spread(tw), stages_ms=stages,
                                  count_plane_bytes=cb, emit_plane_bytes_at_most=eb, count_GBps=gbps(cb, stages["tsdf_count"]),
                                  emit_GBps_at_most=gbps(eb, stages.get("tsdf_emit", 0.0)))
            print(json.dumps(dict(frame=name, **out)), flush=True)
            rec["volumes"].append(out)
            del s, w, rgb, op, oc
            torch.cuda.empty_cache()
    results["frames"].append(rec)
    e.trim()
    del e, ta, tb, dd, df, dx, col
    torch.cuda.empty_cache()

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
