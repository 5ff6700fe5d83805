"""Child process of tests/test_gpu_feature_walk.py (needs an MI355X): ONE long-lived engine takes its walk of
tests/feature_walk.py twice, plain and then with every buffer poisoned (SGM_OPT_POISON, csrc/sgm_debug.h) in front of the
call that precedes each compute and in front of the compute itself.

    feature_walk_child.py <engine name>

Every step compares bit for bit: every disparity map, the float map and XYZ where asked for, the headroom record, on the
single-pair entries the stage taps, the optional maps through the tap or through the bound tensor as the step draws it (a
tensor that was not bound keeps its marker), and every output of the call in front of the compute against its reference.
The engine's hand-written sequence (feature_walk.sequence_same_frame_other_plan) follows the walk in both passes.  It stops at the first mismatch with the walk so far in the message, and an error return it did not ask for raises: nothing
runs on the device after either.  Prints `FEATURE_WALK_OK <compared steps> <stage names seen>` at the end."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402

import feature_walk as FW  # noqa: E402
import history_child as HC  # noqa: E402
import history_walk as HW  # noqa: E402
import lrc_ref as LR  # noqa: E402
import parity_util as U  # noqa: E402
from oracle import oracle as O  # noqa: E402
from stereo_reconstruction_cv_amd import _lib, synth  # noqa: E402

# Stage names emitted by code that came after history_child.STAGES was written (sgm_engine.hip: run_stage / stage_begin; the
# feature tests pin them one by one).  The eight walks together must see every one of them: a walk that silently took another
# route fails tests/test_gpu_feature_walk.py instead of thinning it.  (The select stage of the split winner-take-all keeps the
# name "wta" and its one launch; that the walks reach it is a condition of tests/test_feature_walks.py, read from the plan.)
NEW_STAGES = ("census", "cost_pix_census", "wta", "wta_conf", "conf",
              "right_fill_invalid", "right_wta", "right_check", "right_median3", "right_speckle",
              "wls_init", "wls_rows", "wls_cols", "wls_final", "lrc_factor", "lrc_match",
              "voxel_count", "voxel_clear", "voxel_insert", "voxel_heads",
              "radius_count", "radius_clear", "radius_insert", "radius_starts", "radius_sort", "radius_query", "radius_compact",
              "stat_count", "stat_clear", "stat_insert", "stat_starts", "stat_sort", "stat_query", "stat_reduce", "stat_keep", "stat_compact",
              "mesh_quads", "mesh_used", "mesh_scan", "mesh_vertices", "mesh_faces", "mesh_normals", "normals_grid")

MARK_F, MARK_B, MARK_U, MARK_CONF, MARK_RIGHT = -77.25, 177, 0xDEADBEEF, 0xEE, -7777
DEVICE_ENTRIES = ("compute_device", "pipeline_device", "pipeline_batch_device")
SGM_ERR_UNSUPPORTED = -4

bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


class Runner(HC.Runner):
    """history_child.Runner with the steps of the feature walks"""

    def fail(self, k, what):
        raise AssertionError(f"step {k}: {what}\n--- walk so far ---\n" + FW.describe(self.name, self.p, self.steps, k))

    # ---- device memory ----
    def dev_in(self, a):
        return None if a is None else self.torch.from_numpy(np.array(a)).to(self.dev)

    def dev_out(self, shape, dtype, mark):
        """a marked output tensor (uint32 as the int32 of the same bits)"""
        a = np.full(shape, mark, dtype)
        return self.torch.from_numpy(a.view(np.int32) if dtype == np.uint32 else a).to(self.dev)

    @staticmethod
    def host_of(t, dtype=None):
        a = t.cpu().numpy()
        return a.view(np.uint32) if dtype == np.uint32 else a

    # ---- the call in front of a compute ----
    def between(self, k, s):
        kind = s["between"]
        if kind in HW.BETWEEN:
            n = self.compared           # (a step counts once here, its call included)
            HC.Runner.between(self, k, s)
            self.compared = n
            return
        x = FW.call_input(s)
        want = FW.call_want(s, x)
        bad = getattr(self, "call_" + kind)(s, s["bopt"], x, want)
        if bad:
            self.fail(k, f"{kind} ({'device' if s['bdev'] else 'host'} entry, {s['bopt']}): " + "; ".join(bad))

    def call_refuse(self, s, b, x, want):
        """a census compute on a 3-channel pair: refused with nothing enqueued and nothing written; the engine stays usable"""
        e, L = self.eng, _lib.load()
        rng = np.random.default_rng(s["bseed"])
        H, W = 12, max(self.p["minDisparity"] + self.p["numDisparities"], 0) - min(self.p["minDisparity"], 0) + 40     # (a frame with a volume)
        a3, b3 = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2))
        disp = np.full((H, W), -7, np.int16)
        e.set_option(_lib.SGM_OPT_COST, FW.CENSUS)
        e.set_option(_lib.SGM_OPT_CHANNELS, 3)
        rc = L.sgm_compute(e._h, a3.ctypes.data, b3.ctypes.data, H, W, 3 * W, disp.ctypes.data)
        msg = _lib.last_error()
        e.set_option(_lib.SGM_OPT_COST, s["opts"]["cost"])
        bad = []
        if rc != SGM_ERR_UNSUPPORTED or "SGM_COST_CENSUS" not in msg:
            bad.append(f"returned {rc} ({msg})")
        if (disp != -7).any():
            bad.append("wrote to the output")
        return bad

    def call_wls(self, s, b, x, want):
        e, t = self.eng, self.torch
        maps, lut, n, H, W = x["maps"], x["lut"], b["n"], b["H"], b["W"]
        single = s["between"] == "wls"
        st = lambda key: None if maps[0][key] is None else np.stack([m[key] for m in maps])
        if not s["bdev"]:
            if single:
                out, outf = e.wls_filter_host(maps[0]["disp"], maps[0]["guide"], maps[0]["conf"], b["invalid"], b["lam"], lut, return_float=True)
                out, outf = [out], [outf]
            else:
                out, outf = e.wls_filter_batch_host(st("disp"), st("guide"), st("conf"), b["invalid"], b["lam"], lut, return_float=True)
        else:
            up = lambda key: None if maps[0][key] is None else [self.dev_in(m[key]) for m in maps]
            d, g, c = up("disp"), up("guide"), up("conf")
            o = [self.dev_out((H, W), np.int16, 77) for _ in maps]
            of = [self.dev_out((H, W), np.float32, 7.0) for _ in maps]
            ptrs = lambda ts: None if ts is None else [v.data_ptr() for v in ts]
            t.cuda.synchronize()
            if single:
                e.wls_filter_device(d[0].data_ptr(), g[0].data_ptr(), b["cn"], None if c is None else c[0].data_ptr(), H, W, b["invalid"],
                                    b["lam"], lut, o[0].data_ptr(), of[0].data_ptr())
            else:
                e.wls_filter_batch_device(ptrs(d), ptrs(g), b["cn"], ptrs(c), H, W, b["invalid"], b["lam"], lut, ptrs(o), ptrs(of))
            e.synchronize()
            out, outf = [self.host_of(v) for v in o], [self.host_of(v) for v in of]
        bad = []
        for i, w in enumerate(want):
            if not np.array_equal(out[i], w["out"]):
                bad.append(f"map {i}: " + U.describe_mismatch("out", np.asarray(out[i]), w["out"]))
            if not np.array_equal(bits(outf[i]), bits(w["out_f32"])):
                bad.append(f"map {i}: the float map differs")
        return bad

    call_wls_batch = call_wls

    def call_lrc(self, s, b, x, want):
        e, t = self.eng, self.torch
        pairs, H, W = x["pairs"], b["H"], b["W"]
        base = lambda q: q["base"] if b["with_base"] else None
        arg = (-16, LR.T_DEFAULT, b["radius"], LR.V_DEFAULT)
        if s["between"] == "lrc" and not s["bdev"]:
            got = [e.lrc_confidence_host(pairs[0]["dl"], pairs[0]["dr"], base(pairs[0]), *arg, want_left=True, want_right=True)]
        else:
            dl, dr = [self.dev_in(q["dl"]) for q in pairs], [self.dev_in(q["dr"]) for q in pairs]
            db = [self.dev_in(q["base"]) for q in pairs] if b["with_base"] else None
            cl, cr = ([self.dev_out((H, W), np.uint8, MARK_B) for _ in pairs] for _ in range(2))
            ptrs = lambda ts: None if ts is None else [v.data_ptr() for v in ts]
            t.cuda.synchronize()
            if s["between"] == "lrc":
                e.lrc_confidence_device(dl[0].data_ptr(), dr[0].data_ptr(), None if db is None else db[0].data_ptr(), H, W, *arg,
                                        cl[0].data_ptr(), cr[0].data_ptr())
            else:
                e.lrc_confidence_batch_device(ptrs(dl), ptrs(dr), ptrs(db), H, W, *arg, ptrs(cl), ptrs(cr))
            e.synchronize()
            got = [(self.host_of(a), self.host_of(c)) for a, c in zip(cl, cr)]
        bad = []
        for i, (w, g) in enumerate(zip(want, got)):
            for side, a, c in (("left", g[0], w[0]), ("right", g[1], w[1])):
                if not np.array_equal(a, c):
                    bad.append(f"pair {i}: " + U.describe_mismatch("conf_" + side, a, c))
        return bad

    call_lrc_batch = call_lrc

    def rows(self, bad, what, got, want, n_rows, mark=None, as_bits=False):
        """the first n_rows rows of an output equal the reference's; the rows behind them keep their marker"""
        if got is None:
            return
        f = bits if as_bits else (lambda a: np.asarray(a))
        if not np.array_equal(f(got[:n_rows]), f(want)):
            bad.append(f"{what} differs")
        if mark is not None and got.shape[0] > n_rows:
            tail, m = got[n_rows:], np.full(1, mark, got.dtype)
            if not (f(tail) == f(m)[0]).all():
                bad.append(f"{what}: rows past the count were written")

    def cloud_call(self, s, x, outs, host, device):
        """the lists of a point-cloud call, through its host or its device entry.  outs: name -> (columns, dtype, marker) of the
        outputs that have n rows.  Returns (dict of whole arrays, what the entry returned besides)."""
        t = self.torch
        n = x["xyz"].reshape(-1, 3).shape[0]
        if not s["bdev"]:
            return host(), None
        dx, dd, dc = self.dev_in(x["xyz"].reshape(-1, 3)), self.dev_in(x["disp"]), self.dev_in(x["colors"])
        o = {nm: self.dev_out((n,) if cols == 1 else (n, cols), dt, mk) for nm, (cols, dt, mk) in outs.items()
             if nm != "colors" or x["colors"] is not None}
        t.cuda.synchronize()
        ptr = lambda v: None if v is None else v.data_ptr()
        ret = device(n, ptr(dx), ptr(dd), ptr(dc), {nm: ptr(o.get(nm)) for nm in outs})
        self.eng.synchronize()
        return {nm: (self.host_of(o[nm], outs[nm][1]) if nm in o else None) for nm in outs}, ret

    def call_voxel(self, s, b, x, want):
        e, bad = self.eng, []
        outs = dict(points=(3, np.float32, MARK_F), colors=(3, np.uint8, MARK_B), counts=(1, np.uint32, MARK_U))
        arg = (b["radius"], (0.0, 0.0, 0.0), b["min_points"])
        g, ret = self.cloud_call(
            s, x, outs, lambda: e.voxel_downsample_host(x["xyz"], x["disp"], x["colors"], *arg, return_counts=True),
            lambda n, dx, dd, dc, o: e.voxel_downsample_device(dx, dd, dc, n, *arg, o["points"], o["colors"], o["counts"]))
        m = want["n_voxels"]
        if ret is None:
            pts, rgb, cnt, noor = g
            if len(pts) != m:
                bad.append(f"{len(pts)} voxels, not {m}")
            g, mark = dict(points=pts, colors=rgb, counts=cnt), False
        else:
            nv, noor = ret
            if nv != m:
                bad.append(f"{nv} voxels, not {m}")
            mark = True
        if noor != want["n_out_of_range"]:
            bad.append(f"{noor} points out of range, not {want['n_out_of_range']}")
        self.rows(bad, "points", g["points"], want["points"], m, MARK_F if mark else None, as_bits=True)
        self.rows(bad, "colors", g["colors"], want["colors"], m, MARK_B if mark else None)
        self.rows(bad, "counts", g["counts"], want["counts"], m, MARK_U if mark else None)
        return bad

    def call_radius(self, s, b, x, want):
        e, bad = self.eng, []
        outs = dict(keep=(1, np.uint8, 99), counts=(1, np.uint32, MARK_U), points=(3, np.float32, MARK_F), colors=(3, np.uint8, MARK_B),
                    index=(1, np.uint32, MARK_U))
        o3 = (0.0, 0.0, 0.0)
        g, ret = self.cloud_call(
            s, x, outs, lambda: e.radius_outlier_host(x["xyz"], x["disp"], x["colors"], b["radius"], b["nb_points"], None, o3,
                                                      return_counts=True, return_index=True),
            lambda n, dx, dd, dc, o: e.radius_outlier_device(dx, dd, dc, n, b["radius"], b["nb_points"], None, o3, o["keep"], o["counts"],
                                                             o["points"], o["colors"], o["index"]))
        m, n = want["n_kept"], want["keep"].shape[0]
        if ret is None:
            pts, rgb, keep, cnt, idx, noor = g
            nk, mark = len(pts), False
            g = dict(points=pts, colors=rgb, keep=keep, counts=cnt, index=idx)
        else:
            (nk, noor), mark = ret, True
        if nk != m or noor != want["n_out_of_range"]:
            bad.append(f"{nk} kept, {noor} out of range, not {m}, {want['n_out_of_range']}")
        self.rows(bad, "keep", g["keep"], want["keep"], n)
        self.rows(bad, "counts", g["counts"], want["counts"], n)
        self.rows(bad, "points", g["points"], want["points"], m, MARK_F if mark else None, as_bits=True)
        self.rows(bad, "colors", g["colors"], want["colors"], m, MARK_B if mark else None)
        self.rows(bad, "index", g["index"], want["index"], m, MARK_U if mark else None)
        return bad

    def call_statistical(self, s, b, x, want):
        e, bad = self.eng, []
        outs = dict(keep=(1, np.uint8, 99), mean=(1, np.float32, MARK_F), points=(3, np.float32, MARK_F), colors=(3, np.uint8, MARK_B),
                    index=(1, np.uint32, MARK_U))
        arg = (b["nb_neighbors"], b["std_ratio"], b["radius"], (0.0, 0.0, 0.0))
        g, ret = self.cloud_call(
            s, x, outs, lambda: e.statistical_outlier_host(x["xyz"], x["disp"], x["colors"], *arg, return_distances=True, return_index=True),
            lambda n, dx, dd, dc, o: e.statistical_outlier_device(dx, dd, dc, n, *arg, o["keep"], o["mean"], o["points"], o["colors"], o["index"]))
        m, n = want["n_kept"], want["keep"].shape[0]
        if ret is None:
            pts, rgb, keep, mean, idx, stats = g
            nk, mark = len(pts), False
            g = dict(points=pts, colors=rgb, keep=keep, mean=mean, index=idx)
        else:
            (nk, stats), mark = ret, True
        if nk != m or stats.tolist() != want["stats"].tolist():
            bad.append(f"{nk} kept, statistics {stats.tolist()}, not {m}, {want['stats'].tolist()}")
        self.rows(bad, "keep", g["keep"], want["keep"], n)
        self.rows(bad, "mean", g["mean"], want["mean"], n, as_bits=True)
        self.rows(bad, "points", g["points"], want["points"], m, MARK_F if mark else None, as_bits=True)
        self.rows(bad, "colors", g["colors"], want["colors"], m, MARK_B if mark else None)
        self.rows(bad, "index", g["index"], want["index"], m, MARK_U if mark else None)
        return bad

    def call_mesh(self, s, b, x, want):
        """sgm_mesh_grid, sgm_normals_grid and sgm_mesh_grid_normals"""
        e, t, bad, kind = self.eng, self.torch, [], s["between"]
        H, W = b["H"], b["W"]
        xyz, disp, col = x["xyz"], x["disp"], x["colors"]
        nfmax = max(2 * max(H - 1, 0) * max(W - 1, 0), 1)
        if kind == "normals":
            if not s["bdev"]:
                img = e.normals_grid_host(xyz, disp, b["max_diff"], b["orient"])
            else:
                dx, dd, dn = self.dev_in(xyz), self.dev_in(disp), self.dev_out((H, W, 3), np.float32, MARK_F)
                t.cuda.synchronize()
                e.normals_grid_device(dx.data_ptr(), dd.data_ptr(), H, W, b["max_diff"], b["orient"], dn.data_ptr())
                e.synchronize()
                img = self.host_of(dn)
            if not np.array_equal(bits(img), bits(want["image"])):
                bad.append(f"{int((bits(img) != bits(want['image'])).any(axis=2).sum())} normals differ")
            return bad
        with_n = kind == "mesh_normals"
        mark = s["bdev"]
        if not s["bdev"]:
            r = e.mesh_grid_normals_host(xyz, disp, col, b["max_diff"], b["orient"]) if with_n else e.mesh_grid_host(xyz, disp, col, b["max_diff"])
            vert, rgb, faces = r[:3]
            nrm = r[3] if with_n else None
            nv, nf = len(vert), len(faces)
        else:
            dx, dd, dc = self.dev_in(xyz), self.dev_in(disp), self.dev_in(col)
            dv, dn = self.dev_out((H * W, 3), np.float32, MARK_F), self.dev_out((H * W, 3), np.float32, MARK_F)
            dr = None if col is None else self.dev_out((H * W, 3), np.uint8, MARK_B)
            df = self.dev_out((nfmax, 3), np.int32, -5)
            ptr = lambda v: None if v is None else v.data_ptr()
            t.cuda.synchronize()
            if with_n:
                nv, nf = e.mesh_grid_normals_device(ptr(dx), ptr(dd), ptr(dc), H, W, b["max_diff"], b["orient"], ptr(dv), ptr(dr), ptr(df), ptr(dn))
            else:
                nv, nf = e.mesh_grid_device(ptr(dx), ptr(dd), ptr(dc), H, W, b["max_diff"], ptr(dv), ptr(dr), ptr(df))
            e.synchronize()
            vert, rgb, faces = self.host_of(dv), None if dr is None else self.host_of(dr), self.host_of(df)
            nrm = self.host_of(dn) if with_n else None
        if (nv, nf) != (want["n_vertices"], want["n_faces"]):
            bad.append(f"{nv} vertices and {nf} faces, not {want['n_vertices']} and {want['n_faces']}")
            return bad
        self.rows(bad, "vertices", vert, want["vertices"], nv, MARK_F if mark else None, as_bits=True)
        self.rows(bad, "colors", rgb, want["colors"], nv, MARK_B if mark else None)
        self.rows(bad, "faces", faces, want["faces"], nf, -5 if mark else None)
        if with_n:
            self.rows(bad, "normals", nrm, want["normals"], nv, MARK_F if mark else None, as_bits=True)
        return bad

    call_normals = call_mesh_normals = call_mesh

    # ---- one step ----
    def run(self, k, s, byte=None):
        t, e, p = self.torch, self.eng, self.p
        H, W, cn, n, o = s["H"], s["W"], s["cn"], s["n"], s["opts"]
        for opt, key in ((_lib.SGM_OPT_SCHEDULE, "schedule"), (_lib.SGM_OPT_SWEEP_ROWS, "sweep_rows"),
                         (_lib.SGM_OPT_PREPASS_ROWS, "prepass_rows"), (_lib.SGM_OPT_CHAIN_WGS, "chain_wgs"),
                         (_lib.SGM_OPT_GROUP_MAX, "group_max"), (_lib.SGM_OPT_KEEP_AGGR, "keep_aggr"),
                         (_lib.SGM_OPT_PROFILE, "profile"), (_lib.SGM_OPT_DEBUG, "debug"), (_lib.SGM_OPT_COST, "cost"),
                         (_lib.SGM_OPT_CONFIDENCE, "confidence"), (_lib.SGM_OPT_RIGHT_VIEW, "right_view")):
            e.set_option(opt, o[key])
        self.poison(byte)
        self.between(k, s)
        if o["profile"] and s["between"] not in ("none", "trim", "refuse"):
            self.seen.update(nm for nm, _, _ in e.stage_times())
        self.poison(byte)
        pairs = [FW.pair(p, s, i) for i in range(n)]
        want = [FW.expected(p, s, i) for i in range(n)]
        maps = [FW.expected_maps(p, s, i) for i in range(n)]
        Q = synth.default_Q(max(W, 2)) if s["with_q"] else None
        entry = s["entry"]
        dispf = xyz = None
        conf_t = right_t = None
        if entry in DEVICE_ENTRIES:      # caller tensors for the optional maps, bound or not: the ones that are not keep their marker
            conf_t = [t.full((H, W), MARK_CONF, dtype=t.uint8, device=self.dev) for _ in range(n)]
            right_t = [t.full((H, W), MARK_RIGHT, dtype=t.int16, device=self.dev) for _ in range(n)]
        ptr = lambda ts: [v.data_ptr() for v in ts]
        if entry == "compute_host":
            disps = [e.compute_host(*pairs[0])]
        elif entry in ("compute_device", "pipeline_device"):
            (dl, pitch), (dr, _) = self.up(pairs[0][0], s["pad"]), self.up(pairs[0][1], s["pad"])
            dd = t.full((H, W), -7, dtype=t.int16, device=self.dev)
            df = t.full((H, W), 9.0, dtype=t.float32, device=self.dev)
            dx = t.full((H, W, 3), 9.0, dtype=t.float32, device=self.dev)
            t.cuda.synchronize()
            kw = dict(d_conf=conf_t[0].data_ptr() if s["bind_conf"] else None, d_rmap=right_t[0].data_ptr() if s["bind_right"] else None)
            if entry == "compute_device":
                e.compute_device(dl.data_ptr(), dr.data_ptr(), H, W, pitch, dd.data_ptr(), cn, **kw)
            else:
                e.pipeline_device(dl.data_ptr(), dr.data_ptr(), H, W, pitch, Q, dd.data_ptr(), df.data_ptr(),
                                  dx.data_ptr() if Q is not None else None, cn, **kw)
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
            e.pipeline_batch_device([a[0].data_ptr() for a, _ in ups], [b[0].data_ptr() for _, b in ups], H, W, pitch, Q, ptr(dd),
                                    ptr(df) if Q is not None else None, ptr(dx) if Q is not None else None, cn,
                                    d_confs=ptr(conf_t) if s["bind_conf"] else None, d_rmaps=ptr(right_t) if s["bind_right"] else None)
            e.synchronize()
            disps = [v.cpu().numpy() for v in dd]
            if Q is not None:
                dispf, xyz = df, dx
        elif entry == "compute_batch_host":        # (no per-pair map from this entry, and it clears a binding)
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
        if ok:
            whr = dict(ok=True, max_cost_plus_p2=max(w["hr"]["max_cost_plus_p2"] for w in want),
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
                v = xyz[i].cpu().numpy() if hasattr(xyz[i], "cpu") else xyz[i]
                ref = O.reproject(O.disp_to_float(np.asarray(w["disp"], np.int16)), Q)
                fin = np.isfinite(ref)
                if not (np.array_equal(np.isfinite(v), fin) and np.array_equal(v[fin], ref[fin])):
                    bad.append(f"pair {i} XYZ differs")
            # the optional maps in the caller's tensors: the reference where bound, the marker where not
            for ts, on, bound, nm, mark in ((conf_t, o["confidence"], s["bind_conf"], "conf", MARK_CONF),
                                            (right_t, o["right_view"], s["bind_right"], "right", MARK_RIGHT)):
                if ts is None:
                    continue
                got = ts[i].cpu().numpy()
                if on and bound:
                    if not np.array_equal(got, maps[i][nm]):
                        bad.append(f"pair {i} bound " + U.describe_mismatch(nm, got, maps[i][nm]))
                elif not (got == (mark if mark >= 0 else np.int16(mark))).all():
                    bad.append(f"pair {i}: the {nm} tensor was not bound and was written")
        # stage taps, taken directly after the compute they belong to (single-pair entries: the engine the caller holds)
        if n == 1 and "batch" not in entry and want[0]["ok"]:
            w = dict(want[0])
            taps = dict(disp_raw=e.tap(_lib.SGM_TAP_DISP_RAW, H, W), disp_median=e.tap(_lib.SGM_TAP_DISP_MEDIAN, H, W))
            if "C" in w:
                taps["C"] = e.tap(_lib.SGM_TAP_COST, H, W)
                if o["keep_aggr"]:
                    taps["S"] = e.tap(_lib.SGM_TAP_AGGR, H, W)
            if o["confidence"] and not s["bind_conf"]:
                taps["conf_raw"], taps["conf"] = e.tap(_lib.SGM_TAP_CONF_RAW, H, W), e.tap(_lib.SGM_TAP_CONF, H, W)
            if o["right_view"]:
                taps["right_raw"] = e.tap(_lib.SGM_TAP_RIGHT_RAW, H, W)
                if not s["bind_right"]:
                    taps["right"] = e.tap(_lib.SGM_TAP_RIGHT, H, W)
            w.update(maps[0])
            for nm, got in taps.items():
                if not np.array_equal(got, w[nm]):
                    bad.append(U.describe_mismatch(nm, got, np.asarray(w[nm])))
        if bad:
            self.fail(k, "\n".join(bad))
        self.compared += 1


def main():
    name = sys.argv[1]
    index = FW.NAMES.index(name)
    # (the hand-written sequence of the engine, where it has one, follows its walk in both passes)
    p, steps = FW.ENGINES[index][1], FW.make_walk(index) + FW.sequence_same_frame_other_plan(name)
    r = Runner(name, p, steps)
    for armed in (False, True):
        for k, s in enumerate(steps):
            r.run(k, s, FW.POISON[k % len(FW.POISON)] if armed else None)
        print(f"walk {name} {'poisoned' if armed else 'plain'}: {len(steps)} steps", flush=True)
    r.eng.set_option(HC.SGM_OPT_POISON, -1)
    print(f"FEATURE_WALK_OK {r.compared} {' '.join(sorted(r.seen))}", flush=True)


if __name__ == "__main__":
    main()
