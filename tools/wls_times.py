#!/usr/bin/env python3
"""What the edge-aware disparity filter costs, on the GPU box: sgm_wls_filter_device on device-resident inputs
at 4K, 1080p and 720p, gray and colour guide, with and without a confidence map.

    tools/wls_times.py [reps [out.json]]        (default output: profiles/wls/times.json)

Per row: `total_ms`, HIP events on the engine's stream around the whole call with SGM_OPT_PROFILE off (two warm-up calls, best of
`reps`), and `stages`, the per-kernel times of SGM_OPT_PROFILE (wls_init, wls_rows, wls_cols, wls_final: the three iterations
added up; best of `reps` each; the event records between the kernels cost some 10 us each, so their sum lies above total_ms).
The figure to hold it against: the pair's own latency-mode compute at 4K D = 256, 10.4 - 10.7 ms (README)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import stereo_reconstruction_cv_amd as cv  # noqa: E402
from stereo_reconstruction_cv_amd import _lib  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "wls", "times.json")
SIZES = [("4K", 2160, 3840), ("1080p", 1080, 1920), ("720p", 720, 1280)]
lut = cv.wls_weights(1.5)
stream = torch.cuda.Stream()
eng = cv.Engine(dict(numDisparities=16), stream=stream.cuda_stream)
results = []
for name, H, W in SIZES:
    rng = np.random.default_rng(H)
    # a piecewise map with noise and 20 % holes over a guide whose levels follow it (the times do not depend on the content:
    # every lane walks its whole line)
    layer = (np.add.outer(np.arange(H) // 97, np.arange(W) // 131) % 3)
    disp = (np.array([200, 420, 600])[layer] + rng.integers(-24, 25, (H, W))).astype(np.int16)
    disp[rng.random((H, W)) < 0.2] = -16
    gray = (np.array([60, 120, 180])[layer] + rng.integers(-2, 3, (H, W))).astype(np.uint8)
    d_disp = torch.from_numpy(disp).cuda()
    d_conf = torch.from_numpy(rng.integers(0, 101, (H, W)).astype(np.uint8)).cuda()
    d_out = torch.empty((H, W), dtype=torch.int16, device="cuda")
    d_outf = torch.empty((H, W), dtype=torch.float32, device="cuda")
    for cn in (1, 3):
        d_guide = torch.from_numpy(gray if cn == 1 else np.ascontiguousarray(np.stack([gray] * 3, axis=-1))).cuda()
        for with_conf in (False, True):
            torch.cuda.synchronize()
            call = lambda: eng.wls_filter_device(d_disp.data_ptr(), d_guide.data_ptr(), cn, d_conf.data_ptr() if with_conf else None, H, W,
                                                 -16, 8000.0, lut, d_out.data_ptr(), d_outf.data_ptr())
            totals, stages = [], {}
            eng.set_option(_lib.SGM_OPT_PROFILE, 0)
            for it in range(2 + reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                call()
                b.record(stream)
                eng.synchronize()
                if it >= 2:
                    totals.append(a.elapsed_time(b))
            eng.set_option(_lib.SGM_OPT_PROFILE, 1)
            for it in range(1 + reps):
                call()
                eng.synchronize()
                if it >= 1:
                    for n, ms, _ in eng.stage_times():
                        stages.setdefault(n, []).append(ms)
            rec = dict(size=name, H=H, W=W, cn=cn, conf=with_conf, total_ms=round(min(totals), 3),
                       total_ms_spread=[round(min(totals), 3), round(max(totals), 3)],
                       stages={n: round(min(v), 3) for n, v in stages.items()}, density_out=round(float((d_out != -16).float().mean()), 4))
            results.append(rec)
            print(json.dumps(rec), flush=True)
    del d_disp, d_conf, d_out, d_outf, d_guide
    eng.trim()
    torch.cuda.empty_cache()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(dict(reps=reps, rows=results), f, indent=1)
