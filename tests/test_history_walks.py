"""What tests/test_gpu_history.py rests on, checked without a GPU: the poison routine of the engine names every device
buffer the engine declares, and the seeded walks stay inside the int16 no-overflow regime often enough to mean something."""
import os
import re

import history_walk as HW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc")


def _engine_devbufs(text):
    """names (and array extents) of the DevBuf members of struct sgm_engine"""
    body = text[text.index("struct sgm_engine {"):]
    body = body[:body.index("\n};")]
    names = []
    for m in re.finditer(r"^\s*DevBuf\s+([^;]+);", body, flags=re.M):
        for decl in m.group(1).split(","):
            names.append(decl.strip())
    return names


def test_poison_routine_names_every_device_buffer_of_the_engine():
    """A DevBuf added to struct sgm_engine later cannot be forgotten: every declared member appears in poison_buffers
    (SGM_OPT_POISON, csrc/sgm_debug.h), an array member with each of its elements, and the one member that is state by
    contract -- chain_err, the sticky give-up flag -- is named there and excluded by name."""
    text = open(os.path.join(CSRC, "sgm_engine.hip")).read()
    decls = _engine_devbufs(text)
    assert len(decls) >= 38 and "io[2][5]" in decls and "chain_err" in decls, decls
    start = text.index("static int poison_buffers(sgm_engine *e, int byte)")
    routine = text[start:text.index("\n}\n", start)]
    for d in decls:
        m = re.fullmatch(r"(\w+)((?:\[\d+\])*)", d)
        assert m, d
        name, dims = m.group(1), [int(x) for x in re.findall(r"\[(\d+)\]", m.group(2))]
        if not dims:
            assert re.search(rf"&e->{name}\b(?!\[)", routine), f"poison_buffers does not name {name}"
            continue
        idx = [[]]
        for n in dims:
            idx = [i + [k] for i in idx for k in range(n)]
        for i in idx:
            el = name + "".join(f"[{k}]" for k in i)
            assert f"&e->{el}" in routine, f"poison_buffers does not name {el}"
    assert "b != &e->chain_err" in routine                       # left alone: neither filled nor re-cleared
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
