#!/usr/bin/env python3
"""What the grid triangulation costs, on the GPU box, in ONE run:

  for the device-resident XYZ image and float disparity of a synthetic 4K D = 256 MODE_HH pair, and of a 1080p D = 128 and a 720p
  D = 64 pair (sgm_pipeline_device with the default Q), sgm_mesh_grid_device with colours at max_diff 0.5, 1 and 4, and on a frame
  of the same size the closed-form ramp (every pixel valid, every quad two triangles: the densest case);
  beside them, in the same run, sgm_compact_points_device on the same cloud and the pair's own compute (sgm_pipeline_device).

    tools/mesh_times.py [reps [out.json]]        (default output: profiles/mesh/times.json)

Times are host wall clock around calls that end in a synchronise (both entries block for their counts), two warm-up calls, median
of `reps` with the spread; with SGM_OPT_PROFILE on in a second pass the stage record (HIP events) splits a mesh call into
mesh_quads / mesh_used / mesh_scan / mesh_vertices / mesh_faces.  Per call: the time as a multiple of the compaction on the same
cloud and as a share of the pair's compute, and the bytes of the call's own model -- reads 16 H W + 3 H W (xyz, disparity, colours),
writes 15 V + 12 F -- and of the work buffers the kernels add (the code byte written once and read by three kernels, the pixel ->
vertex map written and read on V pixels, xyz read a second time for the V vertices), each over the wall clock and over the sum of
the stages as GB/s."""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mesh", "times.json")
SIZES = [("4K D256 HH", 2160, 3840, 256, 1), ("1080p D128 HH", 1080, 1920, 128, 1), ("720p D64 HH", 720, 1280, 64, 1)]
MAX_DIFFS = (0.5, 1.0, 4.0)
med = lambda v: round(statistics.median(v), 4)
spread = lambda v: [round(min(v), 4), round(max(v), 4)]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def byte_model(H, W, V, F):
    n = H * W
    model = 16 * n + 3 * n + 15 * V + 12 * F
    work = n + 3 * n + 4 * V + 4 * V + 12 * V
    return model, work


results = dict(reps=reps, clouds=[])
for name, H, W, D, mode in SIZES:
    a, b = synth.make_pair(H, W, D, 1234)[:2]
    e = cv.Engine(bench.sgbm_params(D, 7, mode))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    n, fmax = H * W, 2 * (H - 1) * (W - 1)
    dd = torch.empty((H, W), dtype=torch.int16, device="cuda")
    df = torch.empty((H, W), dtype=torch.float32, device="cuda")
    dx = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    rgb = torch.from_numpy(np.ascontiguousarray(np.repeat(a[:, :, None], 3, axis=2))).cuda()
    pts = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    oc = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    faces = torch.empty((fmax, 3), dtype=torch.int32, device="cuda")
    Q = synth.default_Q(W)
    # the ramp: every pixel valid, one disparity
    yy = torch.arange(H, device="cuda", dtype=torch.float32).view(H, 1).expand(H, W)
    xx = torch.arange(W, device="cuda", dtype=torch.float32).view(1, W).expand(H, W)
    rx = torch.stack([xx * 0.01, yy * 0.01, torch.full((H, W), 2.0, device="cuda")], dim=2).contiguous()
    rd = torch.full((H, W), 8.0, dtype=torch.float32, device="cuda")

    def compute():
        e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, Q, dd.data_ptr(), df.data_ptr(), dx.data_ptr())
        e.synchronize()

    def compact():
        return e.compact_points_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), n, pts.data_ptr(), oc.data_ptr())

    def mesh(md, x=dx, d=df):
        return e.mesh_grid_device(x.data_ptr(), d.data_ptr(), rgb.data_ptr(), H, W, md, pts.data_ptr(), oc.data_ptr(), faces.data_ptr())

    t_compute = [wall(compute)[0] for _ in range(2 + reps)][2:]
    got = [wall(compact) for _ in range(2 + reps)][2:]
    t_compact, n_valid = [g[0] for g in got], got[0][1]
    rec = dict(cloud=name, H=H, W=W, D=D, mode=mode, pixels=n, valid_points=int(n_valid), compute_ms=med(t_compute),
               compute_spread=spread(t_compute), compact_ms=med(t_compact), compact_spread=spread(t_compact), mesh=[])
    cases = [("max_diff %g" % md, md, dx, df) for md in MAX_DIFFS] + [("ramp", 0.0, rx, rd)]
    for label, md, x, d in cases:
        got = [wall(lambda: mesh(md, x, d)) for _ in range(2 + reps)][2:]
        t, (V, F) = [g[0] for g in got], got[0][1]
        e.set_option(_lib.SGM_OPT_PROFILE, 1)
        runs = []
        for it in range(1 + reps):
            mesh(md, x, d)
            runs.append({k: ms for k, ms, _ in e.stage_times() if k != "_wall"})
        e.set_option(_lib.SGM_OPT_PROFILE, 0)
        stages = {k: med([r[k] for r in runs[1:]]) for k in runs[0]}
        model, work = byte_model(H, W, V, F)
        ms, dev_ms = med(t), round(sum(stages.values()), 4)
        one = dict(case=label, max_diff=md, n_vertices=int(V), n_faces=int(F), faces_of_possible=round(F / fmax, 4), ms=ms, spread=spread(t),
                   stages_ms=stages, stages_sum_ms=dev_ms, over_compaction=round(ms / rec["compact_ms"], 3),
                   share_of_compute=round(ms / rec["compute_ms"], 4), model_MB=round(model / 1e6, 1), work_MB=round(work / 1e6, 1),
                   model_GBps_wall=round(model / ms / 1e6, 1), model_GBps_stages=round(model / dev_ms / 1e6, 1),
                   all_GBps_stages=round((model + work) / dev_ms / 1e6, 1))
        rec["mesh"].append(one)
        print(json.dumps(dict(cloud=name, **one)), flush=True)
    results["clouds"].append(rec)
    print(json.dumps({k: x for k, x in rec.items() if k != "mesh"}), flush=True)
    e.trim()
    del e, ta, tb, dd, df, dx, rgb, pts, oc, faces, rx, rd, xx, yy
    torch.cuda.empty_cache()

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
