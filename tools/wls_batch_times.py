#!/usr/bin/env python3
"""What the batch form of the edge-aware disparity filter costs, on the GPU box: sgm_wls_filter_batch_device
against N sequential sgm_wls_filter_device calls on the same device-resident maps in the same process, at 4K, 1080p and 720p,
gray and colour guide, with a confidence map, lambda 8000, sigma 1.5, the float maps written.

    tools/wls_batch_times.py [reps [out.json]]        (default output: profiles/wls_batch/times.json)

Per row (size, guide, N):  `batch_ms` -- ONE batch call, HIP events on the engine's stream around it, SGM_OPT_PROFILE off, two
warm-up calls, best of `reps`, with the spread and the figure per map;  `single_ms` -- the N single calls between one pair of
events, measured the same way;  `stages` -- the batch call's stage record with SGM_OPT_PROFILE on (wls_init, wls_rows, wls_cols,
wls_final: all chunks and iterations added up; best of 3).  N: 1, 2, 4, 8, 17 at every size, 32 at 1080p and 720p, 64 at 720p.
`variants`: the other shapes of the batched line kernels (csrc/sgm_debug.h: SGM_DBG_WLS_BATCH_*_SHIFT; the first of each list is
the one the library uses) at 4K, N = 17 and at 1080p, N = 64, gray.

Every frame size, and the variants, run in a child process of their own under a time limit; after a child that failed or ran
out of time nothing more is started.  The figure to hold the 4K rows against: the throughput-mode pair time at 4K D = 256,
6.49 - 6.51 ms (README)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"4K": (2160, 3840, (1, 2, 4, 8, 17)), "1080p": (1080, 1920, (1, 2, 4, 8, 17, 32)), "720p": (720, 1280, (1, 2, 4, 8, 17, 32, 64))}
ROWS_SHAPES = ["RW=4 TC=32", "RW=2 TC=64", "RW=1 TC=64", "RW=4 TC=64", "RW=2 TC=32"]     # sgm_engine.hip: wls_rows_shapes
COLS_SHAPES = ["UNR=8", "UNR=16", "UNR=32", "UNR=4"]                                                # ... wls_cols_shapes
CHILD_LIMIT_S = 240


def child(what, reps, out_path):
    sys.path.insert(0, ROOT)
    import torch

    import stereo_reconstruction_cv_amd as cv
    from stereo_reconstruction_cv_amd import _lib

    lut = cv.wls_weights(1.5)
    stream = torch.cuda.Stream()
    eng = cv.Engine(dict(numDisparities=16), stream=stream.cuda_stream)
    dev = torch.device("cuda", eng.device)

    def make_maps(H, W, N, cn):
        """N piecewise maps with noise and 20 % holes over guides whose levels follow them, made on the device (the times do not
        depend on the content: every lane walks its whole line)"""
        g = torch.Generator(device=dev).manual_seed(H + N)
        yy, xx = torch.arange(H, device=dev)[:, None], torch.arange(W, device=dev)[None, :]
        maps = []
        for i in range(N):
            layer = (yy // (97 + i) + xx // (131 + i)) % 3
            disp = (200 + 210 * layer + torch.randint(-24, 25, (H, W), device=dev, generator=g)).to(torch.int16)
            disp[torch.rand((H, W), device=dev, generator=g) < 0.2] = -16
            gray = (60 + 60 * layer + torch.randint(-2, 3, (H, W), device=dev, generator=g)).to(torch.uint8)
            guide = gray if cn == 1 else gray[:, :, None].repeat(1, 1, 3).contiguous()
            conf = torch.randint(0, 101, (H, W), device=dev, generator=g).to(torch.uint8)
            maps.append(dict(disp=disp, guide=guide, conf=conf, out=torch.empty((H, W), dtype=torch.int16, device=dev),
                             outf=torch.empty((H, W), dtype=torch.float32, device=dev)))
        return maps

    def timed(call, n):
        ms = []
        for it in range(2 + n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            eng.synchronize()
            if it >= 2:
                ms.append(a.elapsed_time(b))
        return ms

    def measure(H, W, N, cn, singles=True):
        maps = make_maps(H, W, N, cn)
        p = lambda k: [m[k].data_ptr() for m in maps]
        torch.cuda.synchronize()
        batch = lambda: eng.wls_filter_batch_device(p("disp"), p("guide"), cn, p("conf"), H, W, -16, 8000.0, lut, p("out"), p("outf"))

        def single():
            for m in maps:
                eng.wls_filter_device(m["disp"].data_ptr(), m["guide"].data_ptr(), cn, m["conf"].data_ptr(), H, W, -16, 8000.0, lut,
                                      m["out"].data_ptr(), m["outf"].data_ptr())

        eng.set_option(_lib.SGM_OPT_PROFILE, 0)
        tb = timed(batch, reps)
        rec = dict(batch_ms=round(min(tb), 3), batch_ms_spread=[round(min(tb), 3), round(max(tb), 3)], batch_ms_per_map=round(min(tb) / N, 4))
        if singles:
            ts = timed(single, reps)
            rec.update(single_ms=round(min(ts), 3), single_ms_spread=[round(min(ts), 3), round(max(ts), 3)],
                       single_ms_per_map=round(min(ts) / N, 4), speedup=round(min(ts) / min(tb), 2))
        eng.set_option(_lib.SGM_OPT_PROFILE, 1)
        stages = {}
        for it in range(4):
            batch()
            eng.synchronize()
            if it >= 1:
                for n, ms, _ in eng.stage_times():
                    stages.setdefault(n, []).append(ms)
        eng.set_option(_lib.SGM_OPT_PROFILE, 0)
        rec["stages"] = {n: round(min(v), 3) for n, v in stages.items()}
        rec["density_out"] = round(float((maps[-1]["out"] != -16).float().mean()), 4)
        return rec

    rows = []
    if what == "variants":
        # 4K, N = 17: the batch of the speed condition, every workgroup of a row pass resident at once (578 on 256 CUs);
        # 1080p, N = 64: 1088 workgroups per row pass, more than the 768 the 64-column tile's LDS lets a pass keep resident
        for size, N in (("4K", 17), ("1080p", 64)):
            H, W, _ = SIZES[size]
            for field, shift, names in (("rows", 17, ROWS_SHAPES), ("cols", 20, COLS_SHAPES)):
                for idx, name in enumerate(names):
                    if field == "cols" and idx == 0:
                        continue                     # (rows shape 0 with cols shape 0 is measured once)
                    eng.set_option(_lib.SGM_OPT_DEBUG, idx << shift)
                    rec = dict(kernel=field, shape=name, size=size, H=H, W=W, cn=1, conf=True, N=N, **measure(H, W, N, 1, singles=False))
                    rows.append(rec)
                    print(json.dumps(rec), flush=True)
            eng.set_option(_lib.SGM_OPT_DEBUG, 0)
            eng.trim()
            torch.cuda.empty_cache()
    else:
        H, W, Ns = SIZES[what]
        for cn in (1, 3):
            for N in Ns:
                rec = dict(size=what, H=H, W=W, cn=cn, conf=True, N=N, **measure(H, W, N, cn))
                rows.append(rec)
                print(json.dumps(rec), flush=True)
            eng.trim()
            torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump(rows, f)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "wls_batch", "times.json")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    result = dict(reps=reps, rows=[], variants=[])
    for what in list(SIZES) + ["variants"]:
        part = os.path.abspath(out_path) + f".{what}.part"
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(reps), part], timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            sys.exit(f"wls_batch_times: {what} ran out of its {CHILD_LIMIT_S} s; nothing more is started")
        if r.returncode != 0:
            sys.exit(f"wls_batch_times: {what} ended with status {r.returncode}; nothing more is started")
        with open(part) as f:
            result["variants" if what == "variants" else "rows"] += json.load(f)
        os.remove(part)
        with open(out_path, "w") as f:       # (what is measured so far, should a later step fail)
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
