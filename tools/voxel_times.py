#!/usr/bin/env python3
"""What the voxel-grid downsampling costs, on the GPU box, in ONE run:

  for the device-resident XYZ image of a synthetic 4K D = 256 MODE_HH pair, and of a 1080p D = 128 and a 720p D = 64 pair
  (sgm_pipeline_device with the default Q), sgm_voxel_downsample_device with colours and counts at voxel sizes found by bisection
  so that the cloud reduces to about 10^6, 10^5 and 10^4 voxels, and at one huge voxel that holds every point (the worst case for
  contention) -- each with the wave pre-reduction of k_voxel_insert on and off (SGM_DBG_VOXEL_OTHER_REDUCTION), alternating;
  beside them, in the same run, sgm_compact_points_device on the same cloud and the pair's own compute (sgm_pipeline_device).

    tools/voxel_times.py [reps [out.json]]        (default output: profiles/voxel/times.json)

Times are host wall clock around calls that end in a synchronise (both entries block for their counts), two warm-up calls, median
of `reps` with the spread; with SGM_OPT_PROFILE on in a second pass the stage record (HIP events) splits a voxel call into
voxel_count / voxel_clear / voxel_insert / voxel_heads.  `table_MB` is the table the call clears: 48 bytes per slot, the smallest
power of two of at least twice the points in range."""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "voxel", "times.json")
SIZES = [("4K D256 HH", 2160, 3840, 256, 1), ("1080p D128 HH", 1080, 1920, 128, 1), ("720p D64 HH", 720, 1280, 64, 1)]
TARGETS = (10 ** 6, 10 ** 5, 10 ** 4)
# which k_voxel_insert the library runs without the debug bit (kernels_voxel.h); the bit selects the other one
PRE_IS_DEFAULT = "VOX_PRE_DEFAULT = true" in open(os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc", "kernels_voxel.h")).read()
OTHER = _lib.SGM_DBG_VOXEL_OTHER_REDUCTION
VARIANTS = (("pre", 0 if PRE_IS_DEFAULT else OTHER), ("plain", OTHER if PRE_IS_DEFAULT else 0))
med = lambda v: round(statistics.median(v), 4)
spread = lambda v: [round(min(v), 4), round(max(v), 4)]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


results = dict(reps=reps, library_default="pre" if PRE_IS_DEFAULT else "plain", clouds=[])
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
    ok = torch.empty(n, dtype=torch.int32, device="cuda")
    Q = synth.default_Q(W)

    def compute():
        e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, Q, dd.data_ptr(), df.data_ptr(), dx.data_ptr())
        e.synchronize()

    def compact():
        return e.compact_points_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), n, pts.data_ptr(), oc.data_ptr())

    def voxel(v, origin=(0.0, 0.0, 0.0)):
        return e.voxel_downsample_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), n, v, origin, 1, pts.data_ptr(), oc.data_ptr(),
                                         ok.data_ptr())

    t_compute = [wall(compute)[0] for _ in range(2 + reps)][2:]
    got = [wall(compact) for _ in range(2 + reps)][2:]
    t_compact, n_valid = [g[0] for g in got], got[0][1]
    # voxel sizes by bisection on the count (the count falls as the voxel grows)
    z = dx[:, :, 2].flatten()
    zmed = float(z[torch.isfinite(z) & (df.flatten() > 0)].abs().median())
    sizes = []
    for target in TARGETS:
        lo, hi = zmed * 1e-5, zmed * 10.0
        for _ in range(24):
            mid = (lo * hi) ** 0.5
            nv, _ = voxel(mid)
            lo, hi = (mid, hi) if nv > target else (lo, mid)
            if abs(nv - target) <= 0.03 * target:
                break
        sizes.append(("%.0e voxels" % target, mid, (0.0, 0.0, 0.0)))
    big = 4.0 * float(torch.nan_to_num(dx, nan=0.0, posinf=0.0, neginf=0.0).abs().max()) + 1.0
    sizes.append(("one voxel", big, (-big / 2,) * 3))
    rec = dict(cloud=name, H=H, W=W, D=D, mode=mode, points=n, valid_points=int(n_valid), compute_ms=med(t_compute),
               compute_spread=spread(t_compute), compact_ms=med(t_compact), compact_spread=spread(t_compact), voxel=[])
    for label, v, origin in sizes:
        t = {"pre": [], "plain": []}
        nv = noor = 0
        for it in range(2 + reps):
            for which, bit in VARIANTS:   # alternating: both see the same minute
                e.set_option(_lib.SGM_OPT_DEBUG, bit)
                dt, (nv, noor) = wall(lambda: voxel(v, origin))
                if it >= 2:
                    t[which].append(dt)
        stages = {}
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        for which, bit in VARIANTS:
            e.set_option(_lib.SGM_OPT_DEBUG, bit)
            runs = []
            for it in range(1 + reps):
                voxel(v, origin)
                runs.append({k: ms for k, ms, _ in e.stage_times() if k != "_wall"})
            stages[which] = {k: med([r[k] for r in runs[1:]]) for k in runs[0]}
        e.set_option(_lib.SGM_OPT_PROFILE, 0)
        e.set_option(_lib.SGM_OPT_DEBUG, 0)
        n_in = n_valid - noor      # (valid here is the compaction's: X finite; the few points with a non-finite Y or Z alone are not told apart)
        cap = 1
        while cap < 2 * n_in:
            cap *= 2
        one = dict(case=label, voxel_size=v, n_voxels=int(nv), n_out_of_range=int(noor), table_MB=round(cap * 48 / 2 ** 20, 1),
                   ms={k: med(x) for k, x in t.items()}, spread={k: spread(x) for k, x in t.items()}, stages_ms=stages)
        best = min(one["ms"].values())
        one["over_compaction"] = {k: round(x / rec["compact_ms"], 3) for k, x in one["ms"].items()}
        one["share_of_compute"] = {k: round(x / rec["compute_ms"], 4) for k, x in one["ms"].items()}
        one["faster"] = "pre" if one["ms"]["pre"] == best else "plain"
        rec["voxel"].append(one)
        print(json.dumps(dict(cloud=name, **one)), flush=True)
    results["clouds"].append(rec)
    print(json.dumps({k: x for k, x in rec.items() if k != "voxel"}), flush=True)
    e.trim()
    del e, ta, tb, dd, df, dx, rgb, pts, oc, ok
    torch.cuda.empty_cache()

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
