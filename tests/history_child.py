"""Child process of tests/test_gpu_history.py (needs an MI355X): engines with a HISTORY.

    history_child.py routes   poison invariance: every route make_plan can take and every entry point that owns buffers,
                              each started from buffers filled with a hostile byte (SGM_OPT_POISON, csrc/sgm_debug.h)
    history_child.py walks    the walks of tests/history_walk.py on long-lived engines, once plain and once with the
                              poison switch armed between the steps

Every output, every stage tap that exists and the headroom record are compared bit-exactly with the oracle (MODE_HH4 and
colour: the numpy restatements).  It is a child process because a read-before-write of a buffer that holds indices could
turn poison into a wild address: that ends THIS process, not the test session.  Prints `HISTORY_OK <n>` when everything
ran and matched; a mismatch raises with the whole prefix of the walk in the message."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402

import history_walk as HW  # noqa: E402
import parity_util as U  # noqa: E402
from oracle import oracle as O  # noqa: E402
from stereo_reconstruction_cv_amd import _lib, synth  # noqa: E402
from stereo_reconstruction_cv_amd.stereo import Engine  # noqa: E402

SGM_OPT_POISON = _lib.SGM_OPT_POISON      # csrc/sgm_debug.h: test scaffolding, not part of include/sgm_hip.h

# Every stage name run_compute and the pipeline entries can emit (sgm_engine.hip: run_stage / stage_begin).  The routes
# must reach all of them: a route that silently falls back to another plan then fails the test instead of thinning it.
STAGES = ("features", "features_c3", "cost_pix", "cost_box", "cost_hsum", "cost_hsum_c3", "cost_vsum",
          "prepass_dn", "prepass_up", "sweep_dn", "sweep_up", "sweep_up_wta", "chain_dn", "chain_up", "paths5", "paths4",
          "path_S", "path_SE", "path_SW", "path_N", "path_NE", "path_NW", "path_E", "path_W", "path_W_wta",
          "wta", "select_lr", "median3", "speckle", "fill_invalid", "to_float", "float_xyz")


class Runner:
    """One long-lived engine and the steps it has taken."""

    def __init__(self, name, p, steps):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.name, self.p, self.steps = name, p, steps
        self.eng = Engine(p)
        self.seen = set()       # stage names of the profiled computes
        self.compared = 0

    def fail(self, k, what):
        raise AssertionError(f"step {k}: {what}\n--- walk so far ---\n" + HW.describe(self.name, self.p, self.steps, k))

    def poison(self, byte):
        if byte is not None:
            self.eng.set_option(SGM_OPT_POISON, byte)

    def up(self, a, pad=0):
        """host image -> device tensor whose rows are `pad` bytes longer than they need to be; returns (tensor, row pitch)"""
        t = self.torch
        H = a.shape[0]
        row = a.reshape(H, -1)
        buf = t.full((H, row.shape[1] + pad), 0xA5, dtype=t.uint8, device=self.dev)
        buf[:, :row.shape[1]] = t.from_numpy(np.ascontiguousarray(row)).to(self.dev)
        return buf, row.shape[1] + pad

    # ---- stand-alone entries on host pointers, at shapes that have nothing to do with the last compute ----
    def between(self, k, s):
        b, e = s["between"], self.eng
        rng = np.random.default_rng(s["bseed"])
        H, W = int(rng.integers(1, 90)), int(rng.integers(1, 330))
        d16 = rng.integers(-16, 700, (H, W)).astype(np.int16)
        d16[rng.random((H, W)) < 0.3] = -16
        Q = synth.default_Q(max(W, 2))
        if b == "none":
            return
        if b == "trim":
            e.trim()
        elif b == "median":
            if not np.array_equal(e.median3x3_host(d16), O.median3x3(d16)):
                self.fail(k, f"median3x3 {H}x{W}")
        elif b == "speckles":
            sm = (d16 // 64 * 64).astype(np.int16)      # plateaus: components of many sizes
            for arg in ((4, 7), (30, 16), (100, 512)):
                if not np.array_equal(e.filter_speckles_host(sm, -16, *arg), O.filter_speckles(sm, -16, *arg)):
                    self.fail(k, f"filter_speckles {H}x{W} {arg}")
        elif b == "to_float":
            if not np.array_equal(e.disp_to_float_host(d16).view(np.uint32), O.disp_to_float(d16).view(np.uint32)):
                self.fail(k, f"disp_to_float {H}x{W}")
        elif b in ("reproject", "reproject_missing"):
            f = O.disp_to_float(d16)
            hm = b == "reproject_missing"
            got, ref = e.reproject_host(f, np.ascontiguousarray(Q, np.float64), hm), O.reproject(f, Q, hm)
            fin = np.isfinite(ref)
            if not (np.array_equal(np.isfinite(got), fin) and np.array_equal(got[fin], ref[fin])):
                self.fail(k, f"reproject {H}x{W} handleMissingValues={hm}")
        elif b in ("mask", "compact"):
            f = O.disp_to_float(d16)
            xyz = O.reproject(f, Q)
            mask = O.valid_mask(xyz, f)
            if b == "mask":
                if not np.array_equal(e.valid_mask_host(xyz, f), mask):
                    self.fail(k, f"valid_mask {H}x{W}")
            else:
                rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
                pts, cols = e.compact_points_host(xyz, f, rgb)
                if not (np.array_equal(pts.view(np.uint32), xyz[mask].view(np.uint32)) and np.array_equal(cols, rgb[mask])):
                    self.fail(k, f"compact_points {H}x{W}")
        elif b == "rectify":
            Wr, Hr = max(W, 8), max(H, 8)
            K = np.array([[0.9 * Wr, 0, Wr / 2 - 0.5], [0, 0.91 * Wr, Hr / 2 + 0.25], [0, 0, 1]])
            dist = np.array([0.05, -0.01, 0.001, 0.002, 0.0])
            m1, m2 = e.init_undistort_rectify_map_host(K, dist, None, K, Wr, Hr)
            w1, w2 = O.init_undistort_rectify_map(K, dist, None, K, (Wr, Hr))
            if not (np.array_equal(m1, w1) and np.array_equal(m2, w2)):
                self.fail(k, f"initUndistortRectifyMap {Hr}x{Wr}")
            img = rng.integers(0, 256, (Hr + 3, Wr + 5)).astype(np.uint8)
            if not np.array_equal(e.remap_linear_host(img, m1, m2), O.remap_linear(img, w1, w2)):
                self.fail(k, f"remap {Hr}x{Wr}")
        else:
            raise ValueError(b)
        self.compared += 1

    # ---- one step ----
    def run(self, k, s, byte=None):
        t, e, p = self.torch, self.eng, self.p
        H, W, cn, n, o = s["H"], s["W"], s["cn"], s["n"], s["opts"]
        self.poison(byte)
        self.between(k, s)
        for opt, key in ((_lib.SGM_OPT_SCHEDULE, "schedule"), (_lib.SGM_OPT_SWEEP_ROWS, "sweep_rows"),
                         (_lib.SGM_OPT_PREPASS_ROWS, "prepass_rows"), (_lib.SGM_OPT_CHAIN_WGS, "chain_wgs"),
                         (_lib.SGM_OPT_GROUP_MAX, "group_max"), (_lib.SGM_OPT_KEEP_AGGR, "keep_aggr"),
                         (_lib.SGM_OPT_PROFILE, "profile"), (_lib.SGM_OPT_DEBUG, "debug")):
            e.set_option(opt, o[key])
        self.poison(byte)
        pairs = [HW.pair(p, s, i) for i in range(n)]
        want = [HW.expected(p, s, i) for i in range(n)]
        Q = synth.default_Q(max(W, 2)) if s["with_q"] else None
        entry = s["entry"]
        dispf = xyz = None
        if entry == "compute_host":
            disps = [e.compute_host(*pairs[0])]
        elif entry in ("compute_device", "pipeline_device"):
            (dl, pitch), (dr, _) = self.up(pairs[0][0], s["pad"]), self.up(pairs[0][1], s["pad"])
            dd = t.full((H, W), -7, dtype=t.int16, device=self.dev)
            df = t.full((H, W), 9.0, dtype=t.float32, device=self.dev)
            dx = t.full((H, W, 3), 9.0, dtype=t.float32, device=self.dev)
            t.cuda.synchronize()
            if entry == "compute_device":
                e.compute_device(dl.data_ptr(), dr.data_ptr(), H, W, pitch, dd.data_ptr(), cn)
            else:
                e.pipeline_device(dl.data_ptr(), dr.data_ptr(), H, W, pitch, Q, dd.data_ptr(), df.data_ptr(),
                                  dx.data_ptr() if Q is not None else None, cn)
                dispf = [df]
                xyz = [dx] if Q is not None else None
            e.synchronize()
            disps = [dd.cpu().numpy()]
        elif entry == "pipeline_batch_device":
            ups = [(self.up(a, s["pad"]), self.up(b, s["pad"])) for a, b in pairs]
            pitch = ups[0][0][1]
            dd = [t.full((H, W), -7, dtype=t.int16, device=self.dev) for _ in range(n)]
            df = [t.full((H, W), 9.0, dtype=t.float32, device=self.dev) for _ in range(n)]
            dx = [t.full((H, W, 3), 9.0, dtype=t.float32, device=self.dev) for _ in range(n)]
            t.cuda.synchronize()
            ptr = lambda ts: [x.data_ptr() for x in ts]
            e.pipeline_batch_device([a[0].data_ptr() for a, _ in ups], [b[0].data_ptr() for _, b in ups], H, W, pitch, Q, ptr(dd),
                                    ptr(df) if Q is not None else None, ptr(dx) if Q is not None else None, cn)
            e.synchronize()
            disps = [x.cpu().numpy() for x in dd]
            if Q is not None:
                dispf, xyz = df, dx
        elif entry == "compute_batch_host":
            r = e.compute_batch_host(np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]), Q)
            disps, hx = (r if Q is not None else (r, None))
            disps = list(disps)
            if hx is not None:
                xyz = list(hx)
        else:
            raise ValueError(entry)
        # the engine's own regime record: the whole call's (a batch: the maximum over its pairs)
        hr = e.headroom()
        ok = all(w["ok"] for w in want)
        if hr["ok"] != ok:
            self.fail(k, f"headroom verdict: hip {hr}, expected ok={ok}")
        if all(w["hr"] is not None for w in want):
            whr = dict(ok=ok, max_cost_plus_p2=max(w["hr"]["max_cost_plus_p2"] for w in want),
                       max_delta=max(w["hr"]["max_delta"] for w in want))
            if hr != whr:
                self.fail(k, f"headroom record: hip {hr} != {whr}")
        if o["profile"]:
            self.seen.update(nm for nm, _, _ in e.stage_times())
        bad = []
        for i in range(n):
            w = want[i]
            if not w["ok"]:
                continue            # outside the regime no parity is claimed; the step is history for the next one
            if not np.array_equal(disps[i], w["disp"]):
                bad.append(f"pair {i} " + U.describe_mismatch("disp", disps[i], np.asarray(w["disp"])))
            if dispf is not None:
                f = dispf[i].cpu().numpy()
                if not np.array_equal(f.view(np.uint32), O.disp_to_float(np.asarray(w["disp"], np.int16)).view(np.uint32)):
                    bad.append(f"pair {i} float map differs")
            if xyz is not None:
                x = xyz[i].cpu().numpy() if hasattr(xyz[i], "cpu") else xyz[i]
                ref = O.reproject(O.disp_to_float(np.asarray(w["disp"], np.int16)), Q)
                fin = np.isfinite(ref)
                if not (np.array_equal(np.isfinite(x), fin) and np.array_equal(x[fin], ref[fin])):
                    bad.append(f"pair {i} XYZ differs")
        # stage taps, taken directly after the compute they belong to (single-pair entries: the engine the caller holds)
        if n == 1 and "batch" not in entry and want[0]["ok"]:
            w = want[0]
            taps = dict(disp_raw=e.tap(_lib.SGM_TAP_DISP_RAW, H, W), disp_median=e.tap(_lib.SGM_TAP_DISP_MEDIAN, H, W))
            if "C" in w:
                taps["C"] = e.tap(_lib.SGM_TAP_COST, H, W)
                if o["keep_aggr"]:
                    taps["S"] = e.tap(_lib.SGM_TAP_AGGR, H, W)
            for nm, got in taps.items():
                if not np.array_equal(got, w[nm]):
                    bad.append(U.describe_mismatch(nm, got, np.asarray(w[nm])))
        if bad:
            self.fail(k, "\n".join(bad))
        self.compared += 1


def run_walks():
    total = 0
    for name, p, steps, _ in HW.all_walks():
        for armed in (False, True):
            r = Runner(name, p, steps)
            for k, s in enumerate(steps):
                r.run(k, s, HW.POISON[k % len(HW.POISON)] if armed else None)
            if armed:
                r.eng.set_option(SGM_OPT_POISON, -1)
            total += r.compared
            print(f"walk {name} {'poisoned' if armed else 'plain'}: {len(steps)} steps", flush=True)
            del r
    return total


def routes():
    """(name, parameters, step): each reaches a branch of make_plan or an entry point that owns buffers."""
    S, P = HW.step, U.params
    sp = HW.SP
    R = []
    add = lambda name, p, s: R.append((name, p, s))
    # cost stage: byte cost; int16 pipeline (window 13, preFilterCap 127); k_pix_px (D <= 32); three channels
    add("cost_byte", P(128, 7, 0, 0, **sp), S(40, 400, 1))
    add("cost_int16", P(128, 13, 0, 1, preFilterCap=127, speckleWindowSize=30, speckleRange=2), S(36, 380, 2, debug=256))
    add("cost_pix_px", P(16, 13, 0, 0, **sp), S(40, 200, 3))
    add("cost_c3", P(64, 3, -5, 0, penalty="plain", **sp), S(30, 200, 4, cn=3))
    # path stage, schedule 0: eight directions, five directions
    add("v1_hh", P(128, 5, 0, 1, **sp), S(30, 300, 5, schedule=0))
    add("v1_sgbm", P(256, 5, 0, 0, **sp), S(24, 420, 6, schedule=0))
    # schedule 1: fused pre-pass (many bands, one band), one plain chunk (512), three launches (16)
    for nm, kw in (("fused_prepass", dict(prepass_rows=11, sweep_rows=3)), ("one_band", dict(prepass_rows=11, sweep_rows=64)),
                   ("prepass_one_chunk", dict(prepass_rows=64, sweep_rows=4, debug=512)), ("prepass_3_launches", dict(sweep_rows=5, debug=16)),
                   ("no_overlap", dict(sweep_rows=4, debug=32)), ("fork_early", dict(sweep_rows=4, debug=128)),
                   ("wta_fused", dict(sweep_rows=4, debug=2)), ("wta_separate", dict(sweep_rows=4, debug=2048))):
        add("hh_" + nm, P(128, 5, 0, 1, **sp), S(45, 330, 7, **kw))
        add("sgbm_" + nm, P(256, 5, 0, 0, **sp), S(45, 440, 8, **kw))
    # schedule 2 with 1, 2 and many workgroups
    for wgs in (1, 2, 7):
        add(f"chain_{wgs}", P(128, 7, 0, 1, **sp), S(50, 400, 9, schedule=2, sweep_rows=3, chain_wgs=wgs))
        add(f"chain_sgbm_{wgs}", P(256, 5, 0, 0, **sp), S(50, 440, 10, schedule=2, sweep_rows=4, chain_wgs=wgs))
    # MODE_HH4 in all three schedules and for D <= 64
    for sched in (0, 1, 2):
        add(f"hh4_s{sched}", P(128, 7, 0, 3, **sp), S(37, 211, 11, schedule=sched, sweep_rows=0 if sched == 0 else 4))
        add(f"hh4_small_s{sched}", P(48, 3, 5, 3, penalty="plain", **sp), S(40, 150, 12, schedule=sched))
    # the small-D schedule with 5, 3, 2 and 1 volumes (MODE_HH4 above: 4), and MODE_HH's record form
    for nm, dbg in (("5vol", 0), ("3vol", 8192), ("2vol", 4096), ("1vol", 65536), ("no_lane_groups", 4)):
        add("small_d_" + nm, P(32, 5, 0, 0, **sp), S(40, 260, 13, debug=dbg))
        add("small_d64_" + nm, P(64, 5, 0, 0, **sp), S(33, 300, 14, debug=dbg))
    add("small_d_hh", P(32, 5, 0, 1, **sp), S(40, 260, 15))
    add("small_d_hh_3_launches", P(64, 5, 0, 1, **sp), S(40, 260, 15, debug=16))
    # winner-take-all at other D, fused (2) and separate (2048)
    for D in (48, 80, 160, 336):
        for mode in (0, 1):
            for dbg in (2, 2048):
                add(f"wta_d{D}_m{mode}_{dbg}", P(D, 5, 0, mode, **sp), S(28, D + 130, 16 + D, sweep_rows=4, debug=dbg))
    # speckle filter off; a frame without a volume
    add("no_speckle", P(128, 5, 0, 1, speckleWindowSize=0, speckleRange=0), S(30, 300, 17))
    add("no_volume", P(128, 5, 0, 1, **sp), S(20, 100, 18))
    add("no_volume_hh4", P(64, 5, 0, 3, **sp), S(20, 60, 18))
    # the pipeline and batch entries, schedules 1 and 2, groups smaller than the batch, with and without XYZ
    for sched in (1, 2):
        for q in (True, False):
            kw = dict(schedule=sched, sweep_rows=3, group_max=2, with_q=q)
            add(f"pipeline_s{sched}_q{int(q)}", P(128, 5, 0, 1, **sp), S(40, 330, 19, entry="pipeline_device", **kw))
            add(f"batch_device_s{sched}_q{int(q)}", P(128, 5, 0, 1, **sp), S(40, 330, 20, entry="pipeline_batch_device", n=5, **kw))
            add(f"batch_host_s{sched}_q{int(q)}", P(256, 5, 0, 0, **sp), S(36, 400, 21, entry="compute_batch_host", n=5, **kw))
    add("compute_device", P(128, 5, 0, 1, **sp), S(40, 330, 22, entry="compute_device"))
    # the stand-alone entries on host pointers
    for b in HW.BETWEEN[2:]:
        add("standalone_" + b, P(16, 3, 0, 0, **sp), S(12, 90, 23, between=b))
    return R


def run_routes():
    total = 0
    seen = set()
    for name, p, s in routes():
        r = Runner("route " + name, p, [s] * len(HW.POISON))
        for k, byte in enumerate(HW.POISON):
            r.run(k, s, byte)
        r.eng.set_option(SGM_OPT_POISON, -1)
        seen |= r.seen
        total += r.compared
        del r
    print("stages seen:", " ".join(sorted(seen)), flush=True)
    missing = [nm for nm in STAGES if nm not in seen]
    assert not missing, f"the routes never ran these stages: {missing}"
    return total


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "walks"
    if what == "routes":
        n = run_routes()
    elif what == "walks":
        n = run_walks()
    else:
        raise SystemExit(f"unknown part {what!r}")
    print(f"HISTORY_OK {n}", flush=True)


if __name__ == "__main__":
    main()
