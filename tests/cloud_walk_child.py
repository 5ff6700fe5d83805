"""Child process of tests/test_gpu_cloud_walk.py (needs an MI355X): ONE long-lived engine takes its walk of tests/cloud_walk.py
twice, plain and then with every buffer poisoned (SGM_OPT_POISON, csrc/sgm_debug.h) in front of every call.

    cloud_walk_child.py <engine name>

Every step compares bit for bit what the call's own GPU test compares, through that test's own helpers (the marked outputs of
tests/test_gpu_covariance.py, _dbscan, _plane, _icp and _tsdf; tests/feature_walk_child.py for the older calls and the compute):
every output that was asked for, the statistics and the totals, T, fitness, rmse and the history of a registration, the rows past
a count keeping their marker, the inputs unmodified, the volume's planes after every frame, and on a profiled step the stage
names against _lib.*_STAGES.  The engine's hand-written sequence (cloud_walk.sequence_behind_the_walk) follows the walk in both
passes.  It stops at the first mismatch with the walk so far in the message, and an error return it did not ask for raises:
nothing runs on the device after either.  Prints `CLOUD_WALK_OK <compared steps> <stage names seen>` at the end."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402

import cloud_walk as CW  # noqa: E402
import feature_walk_child as FC  # noqa: E402
import history_child as HC  # noqa: E402
import test_gpu_covariance as TC  # noqa: E402
import test_gpu_dbscan as TD  # noqa: E402
import test_gpu_icp as TI  # noqa: E402
import test_gpu_plane as TP  # noqa: E402
import test_gpu_tsdf as TT  # noqa: E402
import tsdf_ref as TR  # noqa: E402
import stereo_reconstruction_cv_amd as sgm  # noqa: E402
from stereo_reconstruction_cv_amd import _lib  # noqa: E402

u32 = lambda a: np.ascontiguousarray(a).view(np.uint32)


class Runner(FC.Runner):
    """feature_walk_child.Runner with the steps of the cloud walks"""

    def __init__(self, name, index, p, steps):
        super().__init__(name, p, steps)
        self.index = index
        self.planes = None          # the walk's volume, as numpy arrays between the calls
        self.wants = CW.volume_wants(index, steps)

    def fail(self, k, what):
        raise AssertionError(f"step {k}: {what}\n--- walk so far ---\n" + CW.describe(self.name, self.p, self.steps, k))

    def new_pass(self):
        frames = CW.volume_frames(self.index)
        self.planes = TR.empty(CW.DIMS, frames[0]["colors"] is not None)

    # ---- the new calls, through the helpers of their own tests (a mismatch is their AssertionError) ----
    def call_covariance(self, s, a, x, w):
        fn = TC.device if s["dev"] else TC.host
        TC.same(fn(self.eng, x["xyz"], x["disp"], a["radius"], a["k"], a["origin"], a["viewpoint"], bool(a["orient"]), outs=s["outs"]), w)

    def call_dbscan(self, s, a, x, w):
        fn = TD.device if s["dev"] else TD.host
        TD.same(fn(self.eng, x["xyz"], x["disp"], a["radius"], a["k"], a["origin"], outs=s["outs"]), w)

    def call_plane(self, s, a, x, w):
        fn = TP.device if s["dev"] else TP.host
        TP.same(fn(self.eng, x["xyz"], x["disp"], x["colors"], a["t"], a["K"], a["pseed"], a["refine"], a["select"], outs=s["outs"],
                   model=x.get("model")), w)

    call_plane_inliers = call_plane

    def call_icp(self, s, a, x, w):
        entry = "device" if s["dev"] else "host"
        ev = s["kind"] == "evaluate"
        g = TI.call(self.eng, entry, x["src"], x["ds"], x["tgt"], x["dt"], None if ev else x["tn"], a["radius"], 0 if ev else a["est"],
                    0 if ev else a["maxit"], T0=CW.MOTIONS[a["motion"]] if ev else None, origin=a["origin"], outs=s["outs"], evaluate=ev)
        TI.same(g, w, evaluate=ev)

    call_evaluate = call_icp

    def call_transform(self, s, a, x, w):
        e, t = self.eng, self.torch
        xyz, nrm, T = x["xyz"], x["normals"], x["T"]
        if not s["dev"]:
            gx, gn = e.transform_points_host(xyz, T, nrm)
        else:
            tx, tn = self.dev_in(xyz), self.dev_in(nrm)
            ox = tx if a["alias"] else self.dev_out(xyz.shape, np.float32, FC.MARK_F)
            on = None if tn is None else tn if a["alias"] else self.dev_out(nrm.shape, np.float32, FC.MARK_F)
            ptr = lambda v: None if v is None else v.data_ptr()
            t.cuda.synchronize()
            e.transform_points_device(ptr(tx), ptr(tn), xyz.shape[0], T, ptr(ox), ptr(on))
            e.synchronize()
            gx, gn = self.host_of(ox), None if on is None else self.host_of(on)
            if not a["alias"]:
                assert np.array_equal(u32(self.host_of(tx)), u32(xyz)), "the input was written"
        assert np.array_equal(u32(gx), u32(w["points"])), "points"
        assert (gn is None) == (w["normals"] is None) and (gn is None or np.array_equal(u32(gn), u32(w["normals"]))), "normals"

    def call_tsdf_integrate(self, s, a, x, w):
        frame = CW.volume_frames(self.index)[a["frame"]]
        st = TT.integrate(self.eng, "device" if s["dev"] else "host", frame, self.planes, stats=a["stats"])
        assert (st is None) == (not a["stats"]) and (st is None or st.tolist() == w[1].tolist()), (st, w[1])
        TT.same_planes(self.planes, w[0], "the volume")

    def call_tsdf_extract(self, s, a, x, w):
        frame = CW.volume_frames(self.index)[0]
        before = tuple(None if v is None else v.copy() for v in self.planes)
        cap = None if a["count_first"] else w[0].shape[0] + a["extra"]
        got = TT.extract(self.eng, "device" if s["dev"] else "host", frame, self.planes, a["min_weight"], cap, colors=s["colors"])
        TT.same_cloud(got, w[0], w[1], "the volume's crossings")
        TT.same_planes(self.planes, before, "an extraction wrote to the planes")

    def call_compact(self, s, a, x, w):
        e, t = self.eng, self.torch
        xyz, disp, col = x["xyz"], x["disp"], x["colors"]
        n, m = disp.size, w["points"].shape[0]
        if not s["dev"]:
            pts, rgb = e.compact_points_host(xyz, disp, col)
            assert len(pts) == m, (len(pts), m)
            mark = False
        else:
            dx, dd, dc = self.dev_in(xyz), self.dev_in(disp), self.dev_in(col)
            dp = self.dev_out((n, 3), np.float32, FC.MARK_F)
            dr = None if col is None else self.dev_out((n, 3), np.uint8, FC.MARK_B)
            t.cuda.synchronize()
            nv = e.compact_points_device(dx.data_ptr(), dd.data_ptr(), None if dc is None else dc.data_ptr(), n, dp.data_ptr(),
                                         None if dr is None else dr.data_ptr())
            assert nv == m, (nv, m)
            pts, rgb, mark = self.host_of(dp), None if dr is None else self.host_of(dr), True
        bad = []
        self.rows(bad, "points", pts, w["points"], m, FC.MARK_F if mark else None, as_bits=True)
        self.rows(bad, "colors", rgb, w["colors"], m, FC.MARK_B if mark else None)
        assert not bad, bad

    def call_old(self, s, a, x, w):
        """radius, statistical, voxel and mesh_normals as the feature walks call and compare them"""
        kind = s["kind"]
        b = dict(a, **({"H": s["cloud"]["H"], "W": s["cloud"]["W"]} if kind == "mesh_normals" else {}))
        fn = FC.Runner.call_mesh if kind == "mesh_normals" else getattr(FC.Runner, "call_" + kind)
        bad = fn(self, dict(bdev=s["dev"], between=kind), b, x, w)
        assert not bad, "; ".join(bad)

    call_radius = call_statistical = call_voxel = call_mesh_normals = call_old

    def call_refuse(self, s, a, x, w):
        """one argument a new entry refuses: no output and no plane is written, and the engine stays usable"""
        e = self.eng
        entry = "device" if s["dev"] else "host"
        if a["which"] == "icp":             # point-to-plane without normals
            src, ds, tgt, dt, tn = CW.IR.pair_case(65, 300, s["seed"])
            TI.untouched(TI.call(e, entry, src, ds, tgt, dt, None, CW.IR.R_CASE, 1, 2, rc_want=-1))
            assert "sgm_register_icp" in _lib.last_error()
        else:                               # a frame for a volume with front = 0
            frame = dict(CW.volume_frames(self.index)[0], front=0)
            before = tuple(None if v is None else v.copy() for v in self.planes)
            try:
                TT.integrate(e, "host", frame, self.planes)     # (the host entry works on the planes in place)
            except sgm.error as err:
                assert "front" in str(err), err
            else:
                raise AssertionError("front = 0 was not refused")
            TT.same_planes(self.planes, before, "a refused frame wrote to the planes")

    # ---- one step ----
    def stages(self, k, s, x, w):
        """the stage record of a profiled step: names of the call's own, in the order of _lib.*_STAGES"""
        names = [nm for nm, _, _ in self.eng.stage_times() if nm != "_wall"]
        self.seen.update(names)
        kind = s["kind"]
        if kind not in CW.STAGES:
            return
        own = CW.STAGES[kind]
        if [nm for nm in own if nm in names] != names:
            self.fail(k, f"the stage record of {kind} is {names}, not a run through {own}")
        if kind in CW.GRID_USERS and s["empty"] is None and x is not None:
            if CW.capacity(s, w) and names[:5] != list(own[:5]):
                self.fail(k, f"the stage record of {kind} is {names}: the grid's five stages do not lead it")
        if s["empty"] is None and not names:
            self.fail(k, f"a profiled {kind} step left no stage record")

    def run(self, k, s, byte=None):
        e, kind = self.eng, s["kind"]
        if kind == "compute":
            FC.Runner.run(self, k, CW.compute_step(self.p, s), byte)
            return
        e.set_option(_lib.SGM_OPT_PROFILE, s["profile"])
        e.set_option(_lib.SGM_OPT_DEBUG, s["debug"])
        self.poison(byte)
        if kind == "trim":
            e.trim()
            self.compared += 1
            return
        x = CW.call_input(s)
        w = self.wants[k] if kind.startswith("tsdf") else CW.call_want(s, x)
        try:
            getattr(self, "call_" + kind)(s, s["arg"], x, w)
        except AssertionError as err:
            self.fail(k, f"{kind} ({'device' if s['dev'] else 'host'} entry): {err}")
        if s["profile"] and kind != "refuse":
            self.stages(k, s, x, w)
        self.compared += 1


def main():
    name = sys.argv[1]
    index = CW.NAMES.index(name)
    p, walk = CW.ENGINES[index][1], CW.make_walk(index)
    tail = CW.sequence_behind_the_walk(name)
    r = Runner(name, index, p, walk + tail)
    try:
        for armed in (False, True):
            r.new_pass()
            for k, s in enumerate(r.steps):
                r.run(k, s, CW.POISON[k % len(CW.POISON)] if armed else None)
            print(f"walk {name} {'poisoned' if armed else 'plain'}: {len(r.steps)} steps", flush=True)
    finally:
        r.eng.set_option(HC.SGM_OPT_POISON, -1)
    print(f"CLOUD_WALK_OK {r.compared} {' '.join(sorted(r.seen))}", flush=True)


if __name__ == "__main__":
    main()
