#!/usr/bin/env python3
"""What the vertex normals cost, on the GPU box, in ONE run:

  for the device-resident XYZ image and float disparity of a synthetic 4K D = 256 MODE_HH pair, and of a 1080p D = 128 and a 720p
  D = 64 pair (sgm_pipeline_device with the default Q), at max_diff 1, in the same process:
      sgm_mesh_grid_device            the yardstick
      sgm_mesh_grid_normals_device    the same with one normal per vertex: its extra time is what the normals add to a mesh call
      sgm_normals_grid_device         the normal image alone
      sgm_compact_points_device       on the same cloud

    tools/normals_times.py [reps [out.json]]        (default output: profiles/normals/times.json)
    tools/normals_times.py --mesh-only [reps [out.json]]   sgm_mesh_grid_device alone: one series of an A/B of two libraries (SGM_HIP_LIB)

Times are host wall clock around calls that end in a synchronise (the image entry does not block: the engine is synchronised
behind it), two warm-up calls, median of `reps` with the spread; with SGM_OPT_PROFILE on in a second pass the stage record (HIP
events) gives mesh_normals and normals_grid on their own.  The kernel's unique traffic: the image pass reads 12 bytes of xyz and
1 code byte per pixel and writes 12; the list pass reads 1 code byte per pixel, 12 + 4 bytes (point, vertex number) per vertex and
writes 12 per vertex.  Each over its stage time as GB/s."""
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

args = [a for a in sys.argv[1:] if a != "--mesh-only"]
mesh_only = "--mesh-only" in sys.argv[1:]
reps = int(args[0]) if args else 9
out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "normals", "times.json")
SIZES = [("4K D256 HH", 2160, 3840, 256, 1), ("1080p D128 HH", 1080, 1920, 128, 1), ("720p D64 HH", 720, 1280, 64, 1)]
MAX_DIFF = 1.0
med = lambda v: round(statistics.median(v), 4)
spread = lambda v: [round(min(v), 4), round(max(v), 4)]


def wall(e, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    e.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def timed(e, fn):
    got = [wall(e, fn) for _ in range(2 + reps)][2:]
    t = [g[0] for g in got]
    return dict(ms=med(t), spread=spread(t)), got[0][1]


def stages(e, fn):
    e.set_option(_lib.SGM_OPT_PROFILE, 1)
    runs = []
    for _ in range(1 + reps):
        fn()
        runs.append({k: ms for k, ms, _ in e.stage_times() if k != "_wall"})
    e.set_option(_lib.SGM_OPT_PROFILE, 0)
    return {k: med([r[k] for r in runs[1:]]) for k in runs[0]}


results = dict(reps=reps, max_diff=MAX_DIFF, library=os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
               clouds=[])
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
    nrm = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    oc = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    faces = torch.empty((fmax, 3), dtype=torch.int32, device="cuda")
    e.pipeline_device(ta.data_ptr(), tb.data_ptr(), H, W, W, synth.default_Q(W), dd.data_ptr(), df.data_ptr(), dx.data_ptr())
    e.synchronize()

    def mesh():
        return e.mesh_grid_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), H, W, MAX_DIFF, pts.data_ptr(), oc.data_ptr(), faces.data_ptr())

    def mesh_normals():
        return e.mesh_grid_normals_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), H, W, MAX_DIFF, 1, pts.data_ptr(), oc.data_ptr(),
                                          faces.data_ptr(), nrm.data_ptr())

    def image():
        e.normals_grid_device(dx.data_ptr(), df.data_ptr(), H, W, MAX_DIFF, 1, nrm.data_ptr())

    def compact():
        return e.compact_points_device(dx.data_ptr(), df.data_ptr(), rgb.data_ptr(), n, pts.data_ptr(), oc.data_ptr())

    rec = dict(cloud=name, H=H, W=W, D=D, pixels=n)
    rec["mesh_grid"], (V, F) = timed(e, mesh)
    rec.update(n_vertices=int(V), n_faces=int(F))
    if not mesh_only:
        rec["mesh_grid_normals"], (V2, F2) = timed(e, mesh_normals)
        assert (V2, F2) == (V, F)
        rec["normals_grid"], _ = timed(e, image)
        rec["compact_points"], nvalid = timed(e, compact)
        rec["valid_points"] = int(nvalid)
        rec["mesh_grid_again"], _ = timed(e, mesh)          # the yardstick once more, behind the others: the drift of the run
        rec["normals_extra_ms"] = round(rec["mesh_grid_normals"]["ms"] - rec["mesh_grid"]["ms"], 4)
        rec["normals_extra_over_mesh"] = round(rec["normals_extra_ms"] / rec["mesh_grid"]["ms"], 3)
        rec["image_over_mesh"] = round(rec["normals_grid"]["ms"] / rec["mesh_grid"]["ms"], 3)
        st_list, st_img = stages(e, mesh_normals), stages(e, image)
        img_bytes, list_bytes = 25 * n, n + 28 * int(V)
        rec["stages_ms"] = dict(mesh_grid_normals=st_list, normals_grid=st_img)
        rec["kernel"] = dict(image_unique_MB=round(img_bytes / 1e6, 1), image_GBps=round(img_bytes / st_img["normals_grid"] / 1e6, 1),
                             list_unique_MB=round(list_bytes / 1e6, 1), list_GBps=round(list_bytes / st_list["mesh_normals"] / 1e6, 1))
    results["clouds"].append(rec)
    print(json.dumps(rec), flush=True)
    e.trim()
    del e, ta, tb, dd, df, dx, rgb, pts, nrm, oc, faces
    torch.cuda.empty_cache()

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
