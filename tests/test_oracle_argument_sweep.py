"""C oracle vs the numpy restatement (bruteforce_sgbm.py) at the argument edges of argument_edges.py: one deterministic
case per edge, then a seeded random sweep over the fuzz's space widened to all of them.  Every tap is compared.  Cases
that leave the int16 no-overflow regime are skipped, as the GPU fuzz skips them."""
import numpy as np
import pytest

import argument_edges as E
import bruteforce_sgbm as B
from oracle import oracle as O

TAPS = ("C", "S", "disp_raw", "disp_median", "disp")


def _compare(l, r, p):
    """None if the case leaves the regime, else (oracle taps, list of mismatching taps)"""
    d, t = O.sgbm_compute(l, r, taps=True, **p)
    if not t["headroom_ok"]:
        return None
    t["disp"] = d
    b = B.sgbm(l, r, **p)
    bad = []
    for k in TAPS:
        if k not in t:      # (no valid column: the oracle hands out no volumes)
            assert k in ("C", "S") and b[k].size == 0
            continue
        if not np.array_equal(t[k], b[k]):
            bad.append(f"{k}: {int((t[k] != b[k]).sum())} of {t[k].size} differ")
    return t, bad


@pytest.mark.parametrize("name", list(E.EDGES))
def test_edge(name):
    l, r, p = E.edge_case(name)
    res = _compare(l, r, p)
    assert res is not None, "every deterministic edge case stays in the int16 regime"
    t, bad = res
    assert not bad, f"{name} {p}\n" + "\n".join(bad)
    # each case exercises what it is named for
    inv = (p["minDisparity"] - 1) * 16
    if name.startswith("saturated_s"):
        assert (t["S"] == B.MAX_COST).all(axis=2).sum() > 20
    if not E.EDGES[name][4]:
        assert (t["disp_median"] != inv).mean() > 0.2, "degenerate case"


def test_ftzero_wraps_mod_256():
    """At preFilterCap 128 (ftzero 129) the clipped gradient and the border value are bytes: the restatement's planes
    then hold no value above 255, and the value the border columns hold is 129 itself."""
    q = B.normalise(preFilterCap=128)
    img = np.zeros((4, 9), np.uint8)
    img[:, 5:] = 255
    (pf, lo, hi), (raw, _, _) = B._features(img, q["ftzero"])
    assert q["ftzero"] == 129
    assert pf.max() <= 255 and lo.max() <= 255 and hi.max() <= 255
    assert (pf[:, 4] == (129 + 129) % 256).all() and (pf[:, 0] == 129).all() and (raw[:, -1] == 129).all()
    q = B.normalise(preFilterCap=1000)
    (pf, _, _), (raw, _, _) = B._features(img, q["ftzero"])
    assert (pf[:, [0, -1]] == 1001 % 256).all() and (raw[:, [0, -1]] == 1001 % 256).all()
    assert (pf[:, 2] == 1001 % 256).all() and (pf[:, 4] == 2 * 1001 % 256).all()


SWEEP = 800


def test_random_sweep():
    """seeded random cases over the widened space; reports every failing seed at once"""
    failures, compared, sat = [], 0, 0
    for seed in range(SWEEP):
        l, r, p = E.random_case(seed)
        res = _compare(l, r, p)
        if res is None:
            continue
        compared += 1
        t, bad = res
        if "S" in t:
            sat += int((t["S"] == B.MAX_COST).all(axis=2).any())
        if bad:
            failures.append(f"seed {seed} {l.shape} {p}: " + "; ".join(bad))
    assert not failures, f"{len(failures)} of {compared} cases differ:\n" + "\n".join(failures[:20])
    # the sweep is not hollow: most cases stay in the regime, and some saturate a whole S vector
    assert compared >= SWEEP * 2 // 3 and sat >= 3, (compared, sat)


@pytest.mark.parametrize("hm", [False, True])
def test_reproject_dense_Q(hm):
    """Appendix B with a Q that has no zero entry, W exactly 0 at many pixels and rows pinned by pin_xyz_rows: the
    oracle and the restatement agree bit for bit (the signs of inf included), and both differ from the same arithmetic
    with contracted multiply-adds, so an oracle built without -ffp-contract=off fails here."""
    d = E.dense_Q_disparity()
    Q, pins = E.pin_xyz_rows(E.dense_Q(), d)
    assert (E.w_of(Q, d) == 0).sum() >= 30 and (Q != 0).all()
    a, b = O.reproject(d, Q, hm), B.reproject(d, Q, hm)
    assert np.array_equal(a, b, equal_nan=True)
    assert np.isinf(a).any() and np.isfinite(a).mean() > 0.8
    fused = B.reproject(d, Q, hm, fused=True)
    for r, (y, x) in enumerate(pins):       # component r is 0 at its pin without contraction, not 0 with it
        assert b[y, x, r] == 0 and fused[y, x, r] != 0 and np.isfinite(fused[y, x, r]), (r, y, x)
    assert not np.array_equal(a, fused, equal_nan=True)
