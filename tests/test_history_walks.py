"""What tests/test_gpu_history.py rests on, checked without a GPU: the poison routine of the engine names every device
buffer the engine declares, and the seeded walks stay inside the int16 no-overflow regime often enough to mean something."""
import os
import re

import history_walk as HW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc")


def _struct_body(text, name):
    body = text[text.index("struct %s {" % name):]
    return body[:body.index("\n};")]


def _routine(text, head):
    start = text.index(head)
    return text[start:text.index("\n}\n", start)]


def _devbuf_list(text):
    """the entries of SGM_ENGINE_DEVBUFS, as the buffers of an engine e: BUF(name) -> name, ARR(name, dims) -> name + dims,
    MAP(name) -> conf.name and right.name"""
    start = text.index("#define SGM_ENGINE_DEVBUFS(BUF, ARR, MAP)")
    body = re.sub(r"/\*.*?\*/", "", text[start:text.index("\n#define SGM_DEVBUF_DECL(", start)].split("\n", 1)[1], flags=re.S)
    names = []
    for kind, arg in re.findall(r"\b(BUF|ARR|MAP)\(([^)]*)\)", body):
        arg = [a.strip() for a in arg.split(",")]
        names += [arg[0]] if kind == "BUF" else [arg[0] + arg[1]] if kind == "ARR" else ["conf." + arg[0], "right." + arg[0]]
    assert not re.sub(r"\b(BUF|ARR|MAP)\([^)]*\)|[\s\\\\]", "", body), body        # nothing but entries
    return names


def test_poison_routine_names_every_device_buffer_of_the_engine():
    """A DevBuf added to the engine later cannot be forgotten.  Every DevBuf of struct sgm_engine, and of SideMap which it
    holds as conf and right, is declared by ONE list (SGM_ENGINE_DEVBUFS), and by nothing else; poison_buffers (SGM_OPT_POISON,
    csrc/sgm_debug.h), release_buffers and plan_bytes_held walk that list -- members, both SideMaps' members and every element
    of an array member; and the one member that is state by contract -- chain_err, the sticky give-up flag -- is excluded by
    name from the poisoning, and from nothing else."""
    text = open(os.path.join(CSRC, "sgm_engine.hip")).read()
    decls = _devbuf_list(text)
    assert len(decls) >= 38 and len(set(decls)) == len(decls) and "io[2][5]" in decls and "chain_err" in decls, decls
    assert {"conf.raw", "conf.fin", "right.raw", "right.fin"} <= set(decls), decls
    # no DevBuf is declared outside the list: not in sgm_engine, not in a struct it embeds, nowhere in the file -- the only
    # declarators are the two macros, and they are only ever handed to the list, once in sgm_engine and once in SideMap
    assert not re.search(r"^\s*DevBuf\s+\w", text, flags=re.M), "a DevBuf declared outside SGM_ENGINE_DEVBUFS"
    assert len(re.findall(r"^#define \w+\([^)]*\) DevBuf\b", text, flags=re.M)) == 2
    uses = [l.strip() for l in text.splitlines() if "SGM_DEVBUF_DECL" in l and not l.startswith("#define")]
    assert sorted(uses) == ["SGM_ENGINE_DEVBUFS(SGM_DEVBUF_DECL, SGM_DEVBUF_DECL_ARR, SGM_DEVBUF_NONE)",
                            "SGM_ENGINE_DEVBUFS(SGM_DEVBUF_NONE, SGM_DEVBUF_NONE, SGM_DEVBUF_DECL)"], uses
    assert "SGM_ENGINE_DEVBUFS(SGM_DEVBUF_NONE, SGM_DEVBUF_NONE, SGM_DEVBUF_DECL)" in _struct_body(text, "SideMap")
    engine = _struct_body(text, "sgm_engine")
    assert "SGM_ENGINE_DEVBUFS(SGM_DEVBUF_DECL, SGM_DEVBUF_DECL_ARR, SGM_DEVBUF_NONE)" in engine
    assert sorted(re.findall(r"^\s*SideMap\s+(\w+)", engine, flags=re.M)) == ["conf", "right"]   # the two the walk visits
    # the walk reaches every entry: members, both SideMaps, every element of a two-dimensional array
    assert "#define SGM_DEVBUF_VISIT(name) f(e->name);" in text
    assert "#define SGM_DEVBUF_VISIT_ARR(name, dims) for (auto &row : e->name) for (auto &b : row) f(b);" in text
    assert "#define SGM_DEVBUF_VISIT_MAP(name) f(e->conf.name); f(e->right.name);" in text
    assert all(len(re.findall(r"\[\d+\]", d)) == 2 for d in decls if "[" in d), decls
    walk = _routine(text, "static void each_devbuf(E *e, F f)")
    assert "SGM_ENGINE_DEVBUFS(SGM_DEVBUF_VISIT, SGM_DEVBUF_VISIT_ARR, SGM_DEVBUF_VISIT_MAP)" in walk
    # ... and the three routines are that walk
    routine = _routine(text, "static int poison_buffers(sgm_engine *e, int byte)")
    release = _routine(text, "static void release_buffers(sgm_engine *e)")
    held = _routine(text, "static size_t plan_bytes_held(const sgm_engine *e)")
    for r in (routine, release, held):
        assert "each_devbuf(e, [" in r and "&e->" not in r.replace("&e->chain_err", ""), r
    assert "&b != &e->chain_err" in routine                      # left alone: neither filled nor re-cleared
    assert "chain_err" not in release and "chain_err" not in held
    assert "e->g.hr = nullptr" in release
    for behind in ("e->peer", "e->peer2", "e->group"):            # the engines behind it
        assert re.search(rf"poison_buffers\({re.escape(behind)}\b|: {re.escape(behind)}\)", routine), behind
    # armed, DevBuf::ensure fills what it allocates -- on both allocation paths
    ensure = text[text.index("int ensure(size_t bytes)"):text.index("hipError_t release()")]
    assert ensure.count("poison_new()") >= 3, ensure
    # ... and nothing of it reaches the public header or the kernels
    assert "POISON" not in open(os.path.join(ROOT, "include", "sgm_hip.h")).read().upper()
    for h in os.listdir(CSRC):
        if h.startswith("kernels_") or h == "sgm_device.h":
            assert "poison" not in open(os.path.join(CSRC, h)).read().lower(), h


def test_walks_are_reproducible_and_cover_what_they_claim():
    for i, (name, p, colour) in enumerate(HW.ENGINES):
        a, b = HW.make_walk(i), HW.make_walk(i)
        assert a == b and len(a) == HW.STEPS
        D = p["numDisparities"]
        w1 = [HW.width1(p, s["W"]) for s in a]
        assert min(w1) <= 2 and max(w1) >= 150, (name, w1)                   # from nothing matchable to wide
        assert min(s["H"] for s in a) <= 25 and max(s["H"] for s in a) >= 100, name
        assert {s["opts"]["schedule"] for s in a} == {0, 1, 2}, name
        assert len({s["entry"] for s in a}) >= 4, name
        assert any(s["opts"]["debug"] for s in a) and not any(s["opts"]["debug"] & 64 for s in a), name
        if colour:
            assert {s["cn"] for s in a} == {1, 3}, name
        shapes = [(s["H"], s["W"]) for s in a]
        grows = sum(1 for x, y in zip(shapes, shapes[1:]) if y[0] * y[1] > x[0] * x[1])
        assert 3 <= grows <= len(a) - 4, (name, shapes)                        # the walk both grows and shrinks
    modes = {(p["mode"], p["numDisparities"]) for _, p, _ in HW.ENGINES}
    for mode in (0, 1, 3):
        ds = sorted(d for m, d in modes if m == mode)
        assert ds[0] <= 32 and any(d in (48, 64) for d in ds) and 128 in ds and ds[-1] >= 256, (mode, ds)


def test_at_most_one_step_in_eight_of_a_walk_leaves_the_int16_regime():
    """A step whose input leaves the regime is not compared on the GPU (only the engine's verdict is); a walk made of such
    steps would check nothing.  Oracle only: the walks are regenerated here and every pair of every step is computed."""
    for name, p, steps, random_walk in HW.all_walks():
        out = [s["k"] for s in steps if not HW.step_ok(p, s)]
        if random_walk:
            assert 8 * len(out) <= len(steps), (name, out)
        elif name == "out_of_regime_then_in":
            assert [HW.step_ok(p, s) for s in steps] == [False, True] * (len(steps) // 2), name
        else:
            assert not out, (name, out)
