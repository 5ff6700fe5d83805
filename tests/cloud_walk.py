"""Seeded walks of a long-lived engine through the point-cloud calls that came after tests/feature_walk.py was written, and what
every step of them must give (no GPU needed).

The calls walked here share more of the engine than any before them: sgm_covariance_normals, sgm_cluster_dbscan,
sgm_register_icp, the radius and the statistical filter all build their cells through radius_build_grid (rad_ctl, rad_pt, rad_tab,
rad_sorted: a table sized from the points that arrive, none at all where none does), rad_keep is the radius filter's keep byte,
dbscan's core byte and the plane's selection, rad_cnt the counts of two calls, ccount the scan of five, and every host entry
stages through xyz / f32 / crgb_in and cpts / crgb.  A walk is 24 calls on ONE engine: every new kind (covariance, dbscan, plane,
plane_inliers, icp with both estimations, evaluate, transform, tsdf_integrate, tsdf_extract), several of the older sharers of the
same buffers (radius, statistical, voxel, compact, mesh_normals) and the engine events trim, refuse and compute, drawn with
their entry (host or device), their optional inputs and outputs, the profile switch and the A/B bits of sgm_debug.h that act on
the call -- all of which leave the results bit-exact.  Three shapes of step are built on purpose:

  REPLAY            the second step of a pair reuses the cloud of the step before under another kind of call, another radius or
                    another origin: the buffers are sized, and what they hold is another call's
  EMPTY BEHIND FULL a cloud with no point in range (all NaN, no positive disparity, an origin that puts every point out of the
                    cell range, n = 0 through a host entry; n = 1 beside them) directly behind a call that filled the grid
  ONE VOLUME        a TSDF volume of the walk's own lives through it: three integrations and two extractions between the other
                    calls, the expected planes the reference's accumulation of the frames so far

Shared by tests/cloud_walk_child.py (which takes the walks on the GPU) and tests/test_cloud_walks.py (which regenerates them
with the references alone and checks the conditions that keep them meaningful).  Everything is a function of (engine index, walk
seed): a failing walk can be replayed from the step list its failure message prints."""
from __future__ import annotations

import numpy as np

import covariance_ref as CV
import dbscan_ref as DR
import feature_walk as FW
import icp_ref as IR
import normals_ref as NR
import plane_ref as PR
import radius_ref as RR
import statistical_ref as SR
import tsdf_ref as TR
import voxel_ref as VR
from feature_walk import POISON, describe  # noqa: F401
from oracle import oracle as O
from stereo_reconstruction_cv_amd import _lib

F32 = np.float32
# (name, parameters, 3-channel-capable, walk seed): two gray and two colour-capable sets of tests/feature_walk.py, so that the
# computes between the calls differ.  The seeds are the first ones (from 41000 + 101 * index upwards) under which the walk meets
# the conditions of tests/test_cloud_walks.py: if a change to the generator breaks one of them, look for another seed, do not
# loosen the condition.
_SEEDS = (41068, 41102, 41220, 41304)
ENGINES = [FW.ENGINES[j][:3] + (_SEEDS[i],) for i, j in enumerate((0, 1, 3, 5))]
NAMES = [e[0] for e in ENGINES]
STEPS = 24

NEW_KINDS = ("covariance", "dbscan", "plane", "plane_inliers", "icp", "evaluate", "transform", "tsdf_integrate", "tsdf_extract")
OLD_KINDS = ("radius", "statistical", "voxel", "compact", "mesh_normals")
EVENTS = ("trim", "refuse", "compute")
ALL_KINDS = NEW_KINDS + OLD_KINDS + EVENTS
GRID_USERS = ("radius", "statistical", "covariance", "dbscan", "icp")       # who builds cells through radius_build_grid
HOST_AND_DEVICE = NEW_KINDS + OLD_KINDS + ("compute",)
STAGES = dict(covariance=_lib.COVARIANCE_STAGES, dbscan=_lib.DBSCAN_STAGES, plane=_lib.PLANE_STAGES, plane_inliers=_lib.PLANE_STAGES[-2:],
              icp=_lib.ICP_STAGES, evaluate=_lib.ICP_STAGES, tsdf_integrate=_lib.TSDF_STAGES[:1], tsdf_extract=_lib.TSDF_STAGES[1:])

# The A/B bits of these calls (csrc/sgm_debug.h says of each that the results are the same bits under it; none is left out).  Walk
# `index` adds OF_CALL[kind][(index + occurrence) % 4] on a step of that kind: every bit meets the call it acts on and
# SGM_DBG_RADIUS_TIGHT_TABLE, which radius_build_grid reads for all of them, every grid user, whatever the seeds become.
SEP, SEL, GATHER, OTHER, TIGHT = (_lib.SGM_DBG_COV_SEPARATE_SOLVE, _lib.SGM_DBG_COV_SELECT_ACCUM, _lib.SGM_DBG_DBSCAN_GATHER_CORE,
                                  _lib.SGM_DBG_PLANE_OTHER_COUNT, _lib.SGM_DBG_RADIUS_TIGHT_TABLE)
DEBUG_BITS = (SEP, SEL, GATHER, OTHER, TIGHT)
OF_CALL = dict(covariance=(SEP, SEL | TIGHT, SEP | SEL, TIGHT), dbscan=(GATHER, TIGHT, GATHER | TIGHT, 0), plane=(OTHER, 0, OTHER, 0),
               radius=(TIGHT, 0, 0, TIGHT), statistical=(TIGHT, 0, TIGHT, 0), icp=(0, TIGHT, 0, TIGHT))

# sizes: the smallest that still cross the structures (blocks of 256 points, waves of 64, a table of 2 .. 8192 slots)
RANDOM_N = (40, 150, 300, 700, 1500, 3000, 4000)
LAYERED = ((1, 63), (3, 90), (8, 100), (12, 130), (24, 130), (30, 130))
ORGANISED = ((12, 130), (24, 130), (30, 130))          # the clouds of the calls that want layers or an image
PAIR_NS, PAIR_NT = (1, 63, 257, 1000), (300, 1500, 5000)
RADII = (0.03, 0.04, 0.05)
FAR = (1.0e6, -1.0e6, 1.0e6)                            # an origin that leaves every point of these clouds outside the cell range
CAPS = dict(points=4000, ns=1000, nt=5000, max_iteration=3, K=64, dims=(40, 32, 24), frame=(48, 64))
MOTIONS = (np.eye(4), IR.rigid((0, 1, 0), 1.0, (0.01, 0.0, 0.0)), IR.rigid((1, -2, 0.5), 33.0, (0.3, -4.0, 2.5)),
           IR.rigid((3.0, 1.0, 2.0), -1.0, (-0.01, 0.02, 0.01)))
DIMS = (40, 32, 24)
FRAMES = ((48, 64), (24, 32), (48, 64))


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def _draw_cloud(rng, kind):
    ri = lambda lo, hi: int(rng.integers(lo, hi + 1))
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]
    seed = ri(0, 10 ** 6)
    if kind in ("icp", "evaluate"):
        return dict(gen="pair", ns=pick(PAIR_NS), nt=pick(PAIR_NT), seed=seed)
    if kind in ("plane", "plane_inliers", "dbscan", "mesh_normals", "compact", "covariance"):
        H, W = pick(ORGANISED)
        return dict(gen="layered", H=H, W=W, seed=seed)
    if ri(0, 1):
        H, W = pick(LAYERED)
        return dict(gen="layered", H=H, W=W, seed=seed)
    return dict(gen="random", n=pick(RANDOM_N), seed=seed)


def _draw_arg(rng, kind, index):
    ri = lambda lo, hi: int(rng.integers(lo, hi + 1))
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]
    o = (0.0, 0.0, 0.0)
    if kind == "radius":
        return dict(radius=pick(RADII), nb_points=pick((1, 4, 8)), origin=o)
    if kind == "statistical":
        return dict(radius=pick(RADII), nb_neighbors=pick((8, 16, 33)), std_ratio=pick((1.0, 2.0)), origin=o)
    if kind == "voxel":
        return dict(radius=pick(RADII), min_points=pick((1, 2)), origin=o)
    if kind == "covariance":
        return dict(radius=pick(RADII), k=pick((3, 4, 6)), origin=o, viewpoint=pick((o, (1.0, -2.0, 0.5))), orient=ri(0, 1))
    if kind == "dbscan":
        return dict(radius=pick((0.04, 0.05)), k=pick((6, 8)), origin=o)
    if kind in ("plane", "plane_inliers"):
        # (plane_inliers classifies against the model the reference finds with these K and pseed)
        return dict(t=pick((0.03, 0.008)), K=pick((16, 48, 64)), pseed=ri(0, 99), refine=1 if kind == "plane_inliers" else ri(0, 1), select=ri(0, 1))
    if kind == "icp":
        return dict(radius=IR.R_CASE, est=ri(0, 1), maxit=pick((1, 2, 3)), origin=o)
    if kind == "evaluate":
        return dict(radius=IR.R_CASE, motion=pick((0, 1, 3)), origin=o)
    if kind == "transform":
        return dict(motion=pick((1, 2, 3)), normals=bool(index % 3 == 0), alias=bool(index % 4 == 1))
    if kind == "mesh_normals":
        return dict(max_diff=pick(FW.MAX_DIFF), orient=ri(0, 1))
    if kind == "tsdf_extract":
        return dict(min_weight=pick((1, 1, 2)), count_first=bool(ri(0, 1)), extra=pick((0, 1, 300)))
    if kind == "refuse":
        return dict(which=("icp", "tsdf")[index % 2])
    if kind == "compute":
        return dict(H=ri(4, 12), W=ri(20, 60), entry=("pipeline_device", "compute_host")[index % 2], fseed=ri(0, 10 ** 6))
    return {}


OUTS = dict(covariance=("normals", "curvature", "counts", "stats"), dbscan=("labels", "core", "sizes", "stats"),
            plane=("inlier", "distance", "points", "colors", "index", "model", "stats"),
            plane_inliers=("inlier", "distance", "points", "colors", "index"),
            icp=("T", "fitness", "rmse", "corr", "d2", "history", "stats"), evaluate=("fitness", "rmse", "corr", "d2", "stats"))


def _blocks(index, rng):
    """the pairs of walk `index`: (kind, how the second step follows the first)"""
    i = index
    pairs = [[("covariance", None), ("dbscan", "kind")],
             [("plane", None), ("plane_inliers", "kind")],
             [("icp", None), ("evaluate", "kind")],
             [("icp", None), ("icp", "radius" if i % 2 else "empty_origin")],
             [(("voxel", "mesh_normals", "compact", "mesh_normals")[i], None), (("mesh_normals", "voxel", "voxel", "compact")[i], "kind")],
             [(("radius", "statistical")[i % 2], "n1" if i % 2 else None), ("transform", "kind")],
             # a full grid (on one walk of coincident points: every neighbourhood degenerate), a cloud of its own with nothing in
             # it, a full grid behind that, and its cloud once more with nothing in range
             [(("statistical", "covariance", "dbscan", "radius")[i], "identical" if i == 1 else None),
              (("radius", "statistical", "covariance", "dbscan")[i], ("n0", "nan", "nan", "n0")[i]),
              (("dbscan", "covariance", "covariance", "radius")[i], None),
              (("dbscan", "statistical", "covariance", "statistical")[i], ("empty_origin", "empty_disp", "empty_origin", "empty_disp")[i])]]
    return [pairs[int(j)] for j in rng.permutation(len(pairs))]


def make_walk(index: int, seed: int | None = None):
    """The steps of engine ENGINES[index]'s walk: a list of plain dicts."""
    rng = np.random.default_rng(ENGINES[index][3] if seed is None else seed)
    ri = lambda lo, hi: int(rng.integers(lo, hi + 1))
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]
    blocks = _blocks(index, rng)
    # the single steps between the pairs: the volume's five in their order, the three events among them
    where = sorted(int(j) for j in rng.permutation(8)[:5])
    events = [EVENTS[int(j)] for j in rng.permutation(3)]
    tsdf = ["tsdf_integrate", "tsdf_integrate", "tsdf_extract", "tsdf_integrate", "tsdf_extract"]
    singles = [tsdf.pop(0) if j in where else events.pop(0) for j in range(8)]
    order = []
    for j in range(8):
        order.append([(singles[j], None)])
        if j < len(blocks):
            order.append(blocks[j])
    out, occ, icp_est, frame = [], {}, index % 2, 0
    for block in order:
        prev = None
        for kind, how in block:
            n_occ = occ.get(kind, 0)
            occ[kind] = n_occ + 1
            s = dict(k=len(out), kind=kind, dev=bool((index + ALL_KINDS.index(kind) + n_occ) % 2), replay=None, empty=None, cloud=None,
                     arg={}, disp=bool(ri(0, 1)), colors=bool(ri(0, 1)), outs=(), profile=int((n_occ + index) % 2 == 0), debug=0,
                     seed=ri(0, 10 ** 6))
            if how in ("kind", "radius", "empty_origin", "empty_disp"):
                s["cloud"] = dict(prev["cloud"])
                if how == "kind":
                    s.update(replay="kind", arg=_draw_arg(rng, kind, index))
                elif how == "radius":
                    arg = dict(prev["arg"])
                    arg["radius"] = 0.07 if kind == "icp" else pick([r for r in RADII if r != arg["radius"]])
                    s.update(replay="radius", arg=arg, disp=prev["disp"])
                elif how == "empty_origin":
                    same = kind == prev["kind"]
                    arg = dict(prev["arg"]) if same else _draw_arg(rng, kind, index)
                    arg["origin"] = FAR
                    s.update(replay="origin" if same else "kind", empty="origin", arg=arg)
                    if same:
                        s["disp"] = prev["disp"]
                else:
                    s["cloud"]["empty"] = "disp"
                    s.update(replay="kind", empty="disp", arg=_draw_arg(rng, kind, index), disp=True)
            elif how in ("n0", "n1", "nan", "identical"):
                if how == "identical":
                    s["cloud"] = dict(gen="lattice", H=4, W=70, spacing=0.0)
                    how = None
                elif how == "nan":
                    s["cloud"] = dict(_draw_cloud(rng, kind), empty="nan")
                else:
                    s["cloud"] = dict(gen="random", n=int(how[1]), seed=s["seed"])
                    if how == "n0":
                        s["dev"] = False            # (n = 0 through the host entries)
                s.update(empty=how, arg=_draw_arg(rng, kind, index))
            elif kind in ("trim", "refuse", "compute", "tsdf_extract"):
                s["arg"] = _draw_arg(rng, kind, index)
            elif kind == "tsdf_integrate":
                s["arg"] = dict(frame=frame, stats=bool((frame + index) % 2))
                frame += 1
            else:
                s.update(cloud=_draw_cloud(rng, kind), arg=_draw_arg(rng, kind, index))
            if kind == "icp" and how is None:
                s["arg"]["est"] = icp_est           # both estimations in every walk
                icp_est = 1 - icp_est
            if kind in OUTS:
                # which optional outputs are null: one step in two asks for all of them, the others leave one or two out
                outs = list(OUTS[kind])
                if ri(0, 1):
                    for j in sorted({ri(0, len(outs) - 1) for _ in range(ri(1, 2))}, reverse=True):
                        outs.pop(j)
                s["outs"] = tuple(outs)
            s["debug"] = OF_CALL.get(kind, (0,) * 4)[(index + n_occ) % 4]
            if s["debug"] & SEP:
                s["profile"] = 1                    # the stage only this route has
            if kind == "plane":
                s["profile"] = int(index % 2 == 0)
                if s["profile"]:
                    s["arg"]["refine"] = 1          # (the refit's stages, profiled on every other walk; a draw on the others)
            out.append(s)
            prev = s
    assert len(out) == STEPS
    return out


def step(kind, cloud=None, dev=False, disp=True, colors=False, outs=None, profile=0, debug=0, empty=None, seed=1, **arg):
    """A hand-written step (for a named sequence that keeps a found failure covered whatever the seeds become)."""
    assert kind in ALL_KINDS
    return dict(k=-1, kind=kind, dev=dev, replay=None, empty=empty, cloud=cloud, arg=arg, disp=disp, colors=colors,
                outs=tuple(OUTS.get(kind, ()) if outs is None else outs), profile=profile, debug=debug, seed=seed)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
_cache: dict = {}


def _key(s, *more):
    return repr((s["kind"], s["cloud"], s["arg"], s["disp"], s["colors"], s["seed"] if s["kind"] == "transform" else 0) + more)


def cloud_arrays(c):
    """(xyz float32 (n, 3), disp float32 (n) or None, colors uint8 (n, 3) or None) of a cloud: the references' own generators"""
    if c["gen"] == "random":
        xyz, col = RR.random_list(c["n"], c["seed"], extent=0.5)
        disp = None
    elif c["gen"] == "layered":
        xyz, disp, col = RR.layered_lists(c["H"], c["W"], c["seed"])
    elif c["gen"] == "lattice":
        xyz, disp, col = CV.plane_lattice(c["H"], c["W"], c["spacing"]), None, None        # (spacing 0: coincident points)
    else:
        raise ValueError(c)
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    e = c.get("empty")
    if e == "nan":
        xyz = np.full_like(xyz, np.nan)
    elif e == "disp":
        disp = -(np.arange(xyz.shape[0]) % 2).astype(F32)          # 0 and -1: no positive disparity
    return xyz, disp, col


def points_of(c):
    """the number of points a cloud hands to a call (a pair: source, target)"""
    if c["gen"] == "pair":
        return c["ns"], c["nt"]
    return (c["n"] if c["gen"] == "random" else c["H"] * c["W"]),


def call_input(s):
    """the inputs of step s's call: a dict (the volume's steps: see volume_frames)"""
    kind, c, a = s["kind"], s["cloud"], s["arg"]
    if c is None:
        return {}
    if kind in ("icp", "evaluate"):
        src, ds, tgt, dt, tn = IR.pair_case(c["ns"], c["nt"], c["seed"])
        if not s["disp"]:
            ds = dt = None
        return dict(src=src, ds=ds, tgt=tgt, dt=dt, tn=tn)
    xyz, disp, col = cloud_arrays(c)
    x = dict(xyz=xyz, disp=disp if s["disp"] or s["empty"] == "disp" else None,
             colors=col if s["colors"] and kind in ("plane", "plane_inliers", "radius", "statistical", "voxel", "compact", "mesh_normals") else None)
    if kind in ("compact", "mesh_normals"):
        assert c["gen"] == "layered"
        H, W = c["H"], c["W"]
        x = dict(xyz=xyz.reshape(H, W, 3), disp=disp.reshape(H, W), colors=None if x["colors"] is None else col.reshape(H, W, 3))
    if kind == "plane_inliers":
        key = _key(s, "model")
        if key not in _cache:
            _cache[key] = PR.segment(xyz, x["disp"], None, a["t"], a["K"], a["pseed"], True, 0)["model"]
        x["model"] = _cache[key]
    if kind == "transform":
        rng = np.random.default_rng(s["seed"])
        x = dict(xyz=xyz, normals=rng.standard_normal(xyz.shape).astype(F32) if a["normals"] else None, T=MOTIONS[a["motion"]])
    return x


def call_want(s, x, **other):
    """the reference of step s's call on the inputs x = call_input(s) (other: arguments to take instead of the step's).  Cached."""
    kind, a = s["kind"], dict(s["arg"], **other)
    key = _key(s, sorted(other.items()))
    if key in _cache:
        return _cache[key]
    if kind == "radius":
        w = RR.cells(x["xyz"], x["disp"], x["colors"], a["radius"], a["nb_points"], None, a["origin"])
    elif kind == "statistical":
        w = SR.cells(x["xyz"], x["disp"], x["colors"], a["nb_neighbors"], a["std_ratio"], a["radius"], a["origin"])
    elif kind == "voxel":
        w = VR.voxel_downsample(x["xyz"], x["disp"], x["colors"], a["radius"], a["origin"], a["min_points"])
    elif kind == "covariance":
        w = CV.cells(x["xyz"], x["disp"], a["radius"], a["k"], a["origin"], a["viewpoint"], bool(a["orient"]))
    elif kind == "dbscan":
        w = DR.cells(x["xyz"], x["disp"], a["radius"], a["k"], a["origin"])
    elif kind == "plane":
        w = PR.segment(x["xyz"], x["disp"], x["colors"], a["t"], a["K"], a["pseed"], bool(a["refine"]), a["select"])
    elif kind == "plane_inliers":
        w = PR.classify(x["xyz"], x["disp"], x["colors"], x["model"], a["t"], a["select"])
    elif kind == "icp":
        w = IR.register(x["src"], x["ds"], x["tgt"], x["dt"], x["tn"], a["radius"], a["origin"], None, a["est"], a["maxit"])
    elif kind == "evaluate":
        w = IR.register(x["src"], x["ds"], x["tgt"], x["dt"], None, a["radius"], a["origin"], MOTIONS[a["motion"]], 0, 0)
    elif kind == "transform":
        M = IR.m_of(x["T"])
        w = dict(points=IR.transform(M, x["xyz"]), normals=None if x["normals"] is None else IR.transform_normals(M, x["normals"]))
    elif kind == "compact":
        mask = O.valid_mask(x["xyz"], x["disp"])
        w = dict(points=x["xyz"][mask], colors=None if x["colors"] is None else x["colors"][mask])
    elif kind == "mesh_normals":
        w = NR.mesh_grid_normals(x["xyz"], x["disp"], x["colors"], a["max_diff"], a["orient"])
    else:
        w = None
    _cache[key] = w
    return w


def in_range(s, w):
    """points in the cells of a grid user's call, read from the reference's statistics"""
    kind = s["kind"]
    if kind == "radius":
        return int(w["in_range"].sum())
    return int(w["stats"][1 if kind == "icp" else 0])


def capacity(s, w):
    """slots of the table radius_build_grid makes for a grid user's step (0: none is built)"""
    n = in_range(s, w)
    if n == 0:
        return 0
    cap = 1
    while cap < (n if s["debug"] & TIGHT else 2 * n):
        cap *= 2
    return cap


def compute_step(p, s):
    """the feature-walk step of a `compute` step: a small frame that has a volume, through the host or the device entry"""
    a = s["arg"]
    return FW.step(a["H"], max(p["minDisparity"] + p["numDisparities"], 0) - min(p["minDisparity"], 0) + a["W"], a["fseed"],
                   entry=a["entry"], profile=s["profile"])


# ---- the volume of a walk ----------------------------------------------------------------------------------------------------------
def volume_frames(index):
    """the three frames walk `index` integrates into its volume, as dicts of tsdf_ref.case_input: one volume, three cameras"""
    key = ("frames", index)
    if key not in _cache:
        front, color, with_disp = (1 if index < 2 else -1), index % 2 == 0, index % 3 != 1
        out = []
        for j in range(3):
            a = TR.case_input((DIMS, FRAMES[(j + index) % 3], j, front, color, with_disp), seed=10 * index + j)
            a["vs"], a["origin"] = TR.volume_for(DIMS, np.eye(4), front)
            out.append(a)
        _cache[key] = out
    return _cache[key]


def volume_wants(index, steps):
    """step number -> what the volume's step must give: (planes after it, the counts of the frame) of an integration, (points,
    colours) of an extraction -- the reference's accumulation of the frames so far.  Cached, read-only."""
    key = ("volume", index, repr([(s["k"], s["kind"], s["arg"]) for s in steps if s["kind"].startswith("tsdf")]))
    if key not in _cache:
        frames = volume_frames(index)
        pl = TR.empty(DIMS, frames[0]["colors"] is not None)
        out = {}
        for k, s in enumerate(steps):
            if s["kind"] == "tsdf_integrate":
                st = TR.run_case(frames[s["arg"]["frame"]], pl)[1]
                out[k] = (tuple(None if x is None else x.copy() for x in pl), st)
            elif s["kind"] == "tsdf_extract":
                a = frames[0]
                out[k] = TR.extract(DIMS, a["vs"], a["origin"], *pl, s["arg"]["min_weight"])
        _cache[key] = out
    return _cache[key]


# ---- the sequences one would write by hand -----------------------------------------------------------------------------------------
def sequence_behind_the_walk(name):
    """Hand-written steps that run behind the walk of engine `name`, on the same engine and in both passes: the shortest sequence
    that shows a failure a walk found lives here, so that it stays covered whatever the seeds become.  No walk has found one."""
    return []


def all_walks():
    """(name, parameters, steps)"""
    return [(ENGINES[i][0], ENGINES[i][1], make_walk(i)) for i in range(len(ENGINES))]
