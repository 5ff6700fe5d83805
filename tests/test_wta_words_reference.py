"""The deciding half of the split winner-take-all on raw records of lane words (csrc/kernels_path.h: wta_select_words, the
function k_wta_select runs per pixel; here through csrc/sgm_debug.h: sgm_debug_wta_select_n), on the CPU.  The chained second
sweep leaves per pixel {minS << 16 | nq << 6 | ln, w0, w1, pv >> 16 | nx << 16}: the first lane that holds a minimum, that
lane's registers and the facing halves of its neighbours'.  The records are formed here in numpy from that layout, for
random cost vectors and for planted ones that put the best disparity at every position of a lane, and what the function makes
of them must be upstream's selection taken literally (tests/test_wta_split_reference.py: _per_d_form)."""
import ctypes as C

import numpy as np
import pytest

from stereo_reconstruction_cv_amd import _lib
from test_wta_split_reference import _per_d_form, _vectors

RATIOS = (0, 1, 10, 50, 99)


def _planted(D, rng):
    """the best d at every position of a lane, in lanes 0, 1, 62, 63 and a few between; ties inside a lane and across lanes"""
    nh = D // 64                                   # halves (disparities) per lane: 2 NP
    rows = []

    def base():
        return rng.integers(1000, 32768, D, dtype=np.int32)

    for lane in (0, 1, 2, 31, 32, 62, 63):
        for k in range(nh):                        # k = 0 and k = nh - 1: a neighbour sits in the next lane
            for lo in (0, 7, 999):
                s = base()
                s[lane * nh + k] = lo
                rows.append(s)
                t = s.copy()                       # neighbours close to the minimum: they decide `near`
                if lane * nh + k > 0:
                    t[lane * nh + k - 1] = lo + 1
                if lane * nh + k + 1 < D:
                    t[lane * nh + k + 1] = lo + 2
                rows.append(t)
            for k2 in range(k + 1, nh):            # two equal minima inside one lane: the first wins
                s = base()
                s[lane * nh + k] = s[lane * nh + k2] = 5
                rows.append(s)
        for lane2 in (3, 40, 63):                  # equal minima in two lanes: the lower lane wins, whatever the positions
            if lane2 <= lane:
                continue
            for k in range(nh):
                for k2 in range(nh):
                    s = base()
                    s[lane * nh + k] = s[lane2 * nh + k2] = 11
                    rows.append(s)
    return np.stack(rows)


def _raw_records(S, wgt, rng):
    """the records the reducing sweep stores, from the layout"""
    n, D = S.shape
    nh = D // 64
    S = S.astype(np.int64)
    lanes = S.reshape(n, 64, nh)
    minS = S.min(axis=1)
    ln = (lanes.min(axis=2) == minS[:, None]).argmax(axis=1)          # first lane that holds a minimum
    t1 = np.minimum((100 * minS - 1) // wgt + 1, 0x8000)
    nq = (S < t1[:, None]).sum(axis=1)
    rows = np.arange(n)
    w = lanes[rows, ln]                                               # (n, nh) halves of lane ln in d order
    garbage = lambda: rng.integers(0, 1 << 32, n, dtype=np.int64)
    w0 = w[:, 0] | (w[:, 1] << 16)
    w1 = (w[:, 2] | (w[:, 3] << 16)) if nh == 4 else garbage()        # NP = 1: not used
    g = garbage()
    below = np.where(ln > 0, S[rows, np.maximum(ln * nh - 1, 0)], g & 0xffff)             # high half of lane ln - 1's last register
    above = np.where(ln < 63, S[rows, np.minimum((ln + 1) * nh, D - 1)], (g >> 16) & 0xffff)   # low half of lane ln + 1's first
    raw = np.stack([(minS << 16) | (nq << 6) | ln, w0, w1, below | (above << 16)], axis=1)
    return np.ascontiguousarray(raw.astype(np.uint32))


def _select(D, ratio, raw):
    out = np.zeros((len(raw), 2), np.uint32)
    rc = _lib.load().sgm_debug_wta_select_n(D, ratio, raw.ctypes.data_as(C.c_void_p), len(raw), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, (rc, _lib.last_error())
    return out


@pytest.mark.parametrize("D", [128, 256])
def test_select_on_lane_words_equals_the_per_d_form(D):
    rng = np.random.default_rng(20261 + D)
    S = np.concatenate([_vectors(D, 52_000, rng), _planted(D, rng)])
    assert len(S) >= 50_000 + 1000                                    # two values of D: at least 100 000 vectors
    rows = np.arange(len(S))
    for ratio in RATIOS:
        wgt = 100 - ratio
        best, minS, rej = _per_d_form(S, wgt)
        rej = rej | (minS == 32767)
        want_key = np.where(rej, 0xffffffff, (minS.astype(np.int64) << 16) | best).astype(np.uint32)
        want_nb = (S[rows, np.maximum(best - 1, 0)].astype(np.int64) | (S[rows, np.minimum(best + 1, D - 1)].astype(np.int64) << 16)).astype(np.uint32)
        got = _select(D, ratio, _raw_records(S, wgt, rng))
        bad = np.nonzero(got[:, 0] != want_key)[0]
        assert bad.size == 0, (D, ratio, int(bad[0]), hex(int(got[bad[0], 0])), hex(int(want_key[bad[0]])), S[bad[0]].tolist())
        bad = np.nonzero(got[:, 1] != want_nb)[0]
        assert bad.size == 0, (D, ratio, int(bad[0]), hex(int(got[bad[0], 1])), hex(int(want_nb[bad[0]])), S[bad[0]].tolist())
        unsat = minS != 32767
        if ratio > 0:
            assert 0 < (rej & unsat).sum() and (~rej).sum() > 0, (D, ratio)      # both outcomes occur
        else:                                                         # S[d] * 100 < 100 minS never holds
            assert (rej & unsat).sum() == 0


def test_planted_cases_cover_every_position_of_a_lane():
    """what the planted vectors are for: the best d at every residue modulo 2 NP, in lane 0 and in lane 63, first and last d"""
    for D in (128, 256):
        nh = D // 64
        P = _planted(D, np.random.default_rng(3))
        best = P.argmin(axis=1)
        for lane in (0, 63):
            assert {int(b) % nh for b in best[best // nh == lane]} == set(range(nh)), (D, lane)
        assert 0 in best and D - 1 in best


def test_select_refuses_what_the_split_form_never_meets():
    L = _lib.load()
    raw = np.zeros((1, 4), np.uint32)
    out = np.zeros((1, 2), np.uint32)
    a, b = raw.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for D in (64, 192, 512, 0):
        assert L.sgm_debug_wta_select_n(D, 10, a, 1, b) != 0
    for ratio in (-1, 100, 1000):
        assert L.sgm_debug_wta_select_n(256, ratio, a, 1, b) != 0
    assert L.sgm_debug_wta_select_n(256, 10, a, 1, b) == 0 and L.sgm_debug_wta_select_n(128, 0, a, 0, b) == 0
