"""Arithmetic of the split winner-take-all (csrc/kernels_path.h: wta_reduce_pixels, csrc/kernels_post.h: k_wta_select), on
the CPU.  Upstream's uniqueness test rejects a pixel iff some d with |d - best| > 1 has S[d] * wgt < 100 * minS
(wgt = 100 - uniquenessRatio; SURVEY.md A.6, oracle/sgbm_oracle.c).  The split form turns the product into a threshold
T1 = floor((100 minS - 1) / wgt) + 1 taken from an integer reciprocal, and the existence test into a comparison of two
counts.  Both steps are checked here for every input the kernels can meet."""
import numpy as np

from stereo_reconstruction_cv_amd import _lib


def test_threshold_from_the_integer_reciprocal_is_exact_for_every_cost_and_ratio():
    L = _lib.load()
    minS = np.arange(0, 32768, dtype=np.int64)
    for ratio in range(100):
        wgt = 100 - ratio
        want = (100 * minS - 1) // wgt + 1          # floor division: 0 for minS = 0, where no S[d] * wgt < 0 exists
        got = np.fromiter((L.sgm_debug_uniq_threshold(int(m), ratio) for m in minS), dtype=np.int64, count=minS.size)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (ratio, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    assert L.sgm_debug_uniq_threshold(5, 100) == -1 and L.sgm_debug_uniq_threshold(32768, 10) == -1


def _per_d_form(S, wgt):
    """upstream, literally: (first best d, minS, rejected)"""
    D = S.shape[1]
    best = S.argmin(axis=1)                         # first minimum
    minS = S[np.arange(len(S)), best]
    d = np.arange(D)[None, :]
    far = np.abs(d - best[:, None]) > 1
    rej = ((S * wgt < (100 * minS)[:, None]) & far).any(axis=1)
    return best, minS, rej


def _count_form(S, wgt):
    """what the sweep and k_wta_select compute between them"""
    D = S.shape[1]
    best = S.argmin(axis=1)
    minS = S[np.arange(len(S)), best]
    t1 = np.minimum((100 * minS - 1) // wgt + 1, 0x8000)     # the kernels' clamp: S <= 0x7fff
    nq = (S < t1[:, None]).sum(axis=1)
    rows = np.arange(len(S))
    sm = S[rows, np.maximum(best - 1, 0)]
    sp = S[rows, np.minimum(best + 1, D - 1)]
    near = (minS < t1).astype(np.int64) + ((best > 0) & (sm < t1)) + ((best + 1 < D) & (sp < t1))
    return best, minS, nq > near


def _vectors(D, n, rng):
    """random cost vectors with the cases that matter: ties, all equal, the minimum at either end, values at T and T + 1"""
    S = rng.integers(0, 32768, (n, D), dtype=np.int32)
    k = n // 8
    S[:k] = rng.integers(0, 40, (k, D))                                   # many ties, also for the minimum
    S[k:2 * k] = rng.integers(0, 32768, (k, 1))                           # all equal
    S[2 * k:3 * k, 0] = 0                                                 # minimum at 0 ...
    S[3 * k:4 * k, D - 1] = 0                                             # ... and at D - 1 (unless a 0 comes earlier)
    S[4 * k:5 * k] = 32767                                                # saturated everywhere
    S[5 * k:6 * k] = rng.integers(100, 400, (k, D))                       # a narrow band: many values near the threshold
    return S


def test_count_form_equals_the_per_d_form():
    rng = np.random.default_rng(20260)
    total = 0
    for D in (128, 256):
        S = _vectors(D, 50_000, rng)
        for ratio in (0, 1, 10, 50, 99):
            wgt = 100 - ratio
            T = S.copy()
            # plant values exactly at T = T1 - 1 (passes the test) and at T + 1 = T1 (does not), far from and next to the best
            best, minS, _ = _per_d_form(T, wgt)
            t1 = (100 * minS - 1) // wgt + 1
            rows = np.arange(len(T))
            for off, val in ((5, t1 - 1), (9, t1), (1, t1 - 1), (-1, t1)):
                d = (best + off) % D
                ok = (val > minS) & (val <= 32767) & (d != best)           # keep minS and the first best d what they are
                T[rows[ok], d[ok]] = val[ok]
            b1, m1, r1 = _per_d_form(T, wgt)
            b2, m2, r2 = _count_form(T, wgt)
            assert np.array_equal(b1, b2) and np.array_equal(m1, m2)
            bad = np.nonzero(r1 != r2)[0]
            assert bad.size == 0, (D, ratio, int(bad[0]), T[bad[0]].tolist())
            if ratio > 0:       # (ratio 0: S[d] * 100 < 100 minS never holds -- nothing is rejected, in either form)
                assert 0 < r1.sum() < len(T), (D, ratio)                     # both outcomes occur
            else:
                assert r1.sum() == 0
            total += len(T)
    assert total >= 100_000
