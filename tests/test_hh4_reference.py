"""MODE_HH4 without a GPU: the numpy restatement the GPU tests compare against (tests/bruteforce_hh4.py) against answers
that need no implementation and against the C oracle's cost stage, and the C ABI's view of mode 3 through the built
library (no device needed: sgm_geometry, sgm_algorithmic_bytes)."""
import ctypes as C

import numpy as np
import pytest

import bruteforce_hh4 as HH4
import bruteforce_sgbm as BF
import parity_util as U
from oracle import oracle as O
from stereo_reconstruction_cv_amd import _lib, synth


# ---- (a) known answers -------------------------------------------------------------------------------------------------
def test_constant_pair_gives_zero_disparity():
    img = np.full((24, 64), 100, np.uint8)
    r = HH4.sgbm_hh4(img, img, numDisparities=16, blockSize=3)
    d = r["disp"]
    assert (d[:, :16] == -16).all()          # columns [0, D) can never be matched
    assert (d[:, 16:] == 0).all()            # all costs 0 -> first minimum -> d = 0
    assert (r["S"][..., 0] == 0).all()       # d = 0 costs nothing anywhere (the border columns make other d cost something)
    assert r["max_delta"] == 5               # P2 normalised to max(5, P1 + 1); min_d L_r = 0 everywhere


@pytest.mark.parametrize("k", [1, 5, 11])
def test_pure_shift(k):
    base = synth.texture(40, 128, 5).astype(np.uint8)
    right = np.roll(base, -k, axis=1)
    p = dict(minDisparity=0, numDisparities=16, blockSize=5, P1=200, P2=800, disp12MaxDiff=1, preFilterCap=63,
             uniquenessRatio=0, speckleWindowSize=100, speckleRange=32)
    d = HH4.sgbm_hh4(base, right, **p)["disp"]
    inner = d[8:32, 40:104]
    # the parabola fit may move the answer by 1/16 px where neighbours' costs are asymmetric
    assert (np.abs(inner.astype(int) - 16 * k) <= 1).all()
    assert (inner == 16 * k).mean() > 0.9


def test_four_directions_differ_from_the_other_modes():
    """the composition is not MODE_SGBM's or MODE_HH's sum under another name"""
    l, r, _ = synth.make_pair(24, 72, 16, seed=11)
    p = U.params(16, 3, 0, penalty="plain")
    h4 = HH4.sgbm_hh4(l, r, **p)
    for mode in (0, 1):
        other = BF.sgbm(l, r, **dict(p, mode=mode))
        assert np.array_equal(other["C"], h4["C"])
        assert (other["S"] != h4["S"]).any() and (other["disp"] != h4["disp"]).any()


# ---- (b) the helper's cost stage is the oracle's ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,D,bs,minD,penalty", [(24, 72, 16, 3, 0, "plain"), (30, 100, 32, 5, 0, "plain"),
                                                    (20, 120, 64, 5, -8, "plain"), (22, 150, 48, 7, 5, "notebook")])
def test_sum_is_unchanged_with_the_oracles_block_cost(H, W, D, bs, minD, penalty):
    l, r, _ = synth.make_pair(H, W, D, seed=11)
    p = U.params(D, bs, minD, 1, penalty=penalty)
    _, t = O.sgbm_compute(l, r, taps=True, **p)
    assert t["headroom_ok"]
    own = HH4.sgbm_hh4(l, r, select=False, **p)
    fed = HH4.sgbm_hh4(l, r, C=t["C"], select=False, **p)
    assert np.array_equal(own["C"], t["C"])
    assert np.array_equal(own["S"], fed["S"]) and own["max_delta"] == fed["max_delta"]
    assert own["C"].max() + p["P2"] <= t["max_cost_plus_p2"]   # (the oracle's record also covers the running-sum intermediate)


# ---- (c) C ABI ---------------------------------------------------------------------------------------------------------------
def _params(**kw):
    p = _lib.SgmParams()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_abi_accepts_mode_3_and_refuses_mode_2():
    L = _lib.load()
    a, b = C.c_int(), C.c_int()
    base = dict(minDisparity=0, numDisparities=256, blockSize=7, P1=8 * 3 * 49, P2=32 * 3 * 49, disp12MaxDiff=1,
                preFilterCap=63, uniquenessRatio=10, speckleWindowSize=100, speckleRange=32)
    for mode, want in ((0, 0), (1, 0), (3, 0), (2, -4)):
        p = _params(**dict(base, mode=mode))
        assert L.sgm_geometry(C.byref(p), 3840, C.byref(a), C.byref(b)) == want, mode
        if want == 0:
            assert (a.value, b.value) == (256, 3584)
    assert b"3WAY" in L.sgm_last_error()


def test_algorithmic_bytes_of_mode_3():
    """SURVEY.md 8d with Np = 4: 2 HW + (1 + 3 * 4) V + 10 HW at 2160 x 3840, D = 256"""
    L = _lib.load()
    H, W, D = 2160, 3840, 256
    p = _params(minDisparity=0, numDisparities=D, blockSize=7, P1=8 * 3 * 49, P2=32 * 3 * 49, disp12MaxDiff=1, preFilterCap=63,
                uniquenessRatio=10, speckleWindowSize=100, speckleRange=32, mode=3)
    got = L.sgm_algorithmic_bytes(C.byref(p), H, W, 0)
    V = 2 * H * 3584 * D
    assert got == 2 * H * W + 13 * V + 10 * H * W
    assert abs(got / 1e9 - 51.63) < 0.05
    p2 = _params(numDisparities=D, blockSize=7, mode=2)
    assert L.sgm_algorithmic_bytes(C.byref(p2), H, W, 0) == -1


# ---- (d) ISA of the axis-only kernels (a by-product of the library build, as in tests/test_abi.py) ---------------------------
def _isa():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "stereo_reconstruction_cv_amd", "csrc", "sgm_engine.s")).read()


def _kernels(text):
    import re
    for km in re.finditer(r"^(_Z\w+):\s*; @", text, flags=re.M):
        yield km.group(1), text[km.end():text.index(".Lfunc_end", km.end())].split("\n")


def test_axis_kernels_are_built_and_have_no_waterfall_loops():
    """the check tests/test_abi.py applies to k_sweep / k_prepass3 / k_path, for the kernels of this mode: no buffer
    operation wrapped in a v_readfirstlane / s_and_saveexec loop (a descriptor the compiler could not prove uniform)"""
    import re
    seen = set()
    for name, body in _kernels(_isa()):
        m = re.search(r"k_axis_(sweep|chain|prepass|paths4_g)", name)
        if not m:
            continue
        seen.add(m.group(1))
        n = sum(1 for i, l in enumerate(body) if "s_and_saveexec_b64" in l and re.search(r"buffer_(load|store)", " ".join(body[i + 1:i + 3])))
        assert n == 0, (name, n)
        assert not any(re.search(r"buffer_store_dwordx[34]", l) for l in body), name
    assert seen == {"sweep", "chain", "prepass", "paths4_g"}


def test_axis_sweep_is_a_subset_of_the_four_direction_sweep():
    """steady-state block (16 pixels) of the headline configuration <NP = 2, full waves>: two reductions' worth of
    v_readlane per pixel instead of four, the same loads and stores of C and S, no scalar multiplications, and fewer
    instructions than the four-direction kernel's block"""
    import test_abi as T
    text = _isa()
    for mode in (0, 1):
        for kern, ref in (("k_axis_sweep", f"k_sweepILi2ELb0ELi{mode}ELb1E"), ("k_axis_chain", f"k_sweep_chainILi2ELb0ELi{mode}E")):
            m = T._largest_block_mix(text, f"{kern}ILi2ELb0ELi{mode}E")
            assert m["v_readlane_b32"] == 32 and m["v_writelane_b32"] == 0 and m["s_mul_i32"] == 0, (kern, mode, m)
            assert m["buffer_load_dwordx2"] == (16 if mode == 0 else 32) and m["buffer_store_dwordx2"] == 16, (kern, mode, m)
            assert sum(m.values()) < 0.7 * sum(T._largest_block_mix(text, ref).values()), (kern, mode)
