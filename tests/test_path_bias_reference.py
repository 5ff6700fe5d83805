"""The clamped and biased path state of the chained sweeps (csrc/kernels_path.h: path_elem<.., BIAS>, path_normalise_bias),
as a numpy model of ONE step of the recurrence in both forms.  Not a test of the kernel: it pins the arithmetic the kernel's
comments argue for, in the int16 operations the kernel uses.

Plain form, on the normalised state L(d) = L_r(q, d) - min_k L_r(q, k) >= 0 (32767 = the sentinel beyond both ends):

    t(d) = min( min(L(d-1), L(d+1)) +sat P1,  L(d),  P2 )          v(d) = C(d) + t(d)          L'(d) = v(d) - m,  m = min v

Biased form, B = 32767 - P2, on Lb(d) = min(L(d), P2) + B in [B, 32767], with C - B for C:

    tb(d) = min( min(Lb(d-1), Lb(d+1)) +sat P1,  Lb(d) )           v(d) = (C(d) - B) + tb(d)   Lb'(d) = v(d) +sat (B - m)

Why it is exact.  L enters t only through min(., P2), so min(L, P2) serves as well as L.  The saturating add tops out at
32767 = P2 + B, so min(Lb(d-1), Lb(d+1)) +sat P1 = min(L(d-1) + P1, L(d+1) + P1, P2) + B: a clamped neighbour contributes
P2 + P1 > P2, which the P2 term beats anyway, and the sentinel is "P2 or more" in the biased domain.  The minimum with
Lb(d) = min(L(d), P2) + B gives t(d) + B, so v is the plain form's, bit for bit.  v - m >= 0 and B >= 0: v +sat (B - m)
saturates only upwards, at P2 + B, which is the clamp of the next state."""
import numpy as np
import pytest

SENT = 32767


def _sat(a):
    return np.clip(a, -32768, 32767)


def _neigh(L):
    lo = np.concatenate(([SENT], L[:-1]))
    hi = np.concatenate((L[1:], [SENT]))
    return np.minimum(lo, hi)


def plain_step(C, L, P1, P2):
    t = np.minimum(np.minimum(_sat(_neigh(L) + P1), L), P2)
    v = C + t
    m = int(v.min())
    return v, m, v - m


def biased_step(C, Lb, P1, P2):
    B = SENT - P2
    Cb = ((C - B + 32768) % 65536) - 32768                 # a wrapping 16-bit subtraction, as the kernel's
    t = np.minimum(_sat(_neigh(Lb) + P1), Lb)
    v = ((Cb + t + 32768) % 65536) - 32768                  # and a wrapping add
    m = int(v.min())
    assert -32768 <= B - m <= 32767
    return v, m, _sat(v + (B - m))


def _both(C, L, P1, P2):
    """one step from the normalised state L in both forms; returns v and the two next states"""
    B = SENT - P2
    v, m, Ln = plain_step(C, L, P1, P2)
    vb, mb, Lbn = biased_step(C, np.minimum(L, P2) + B, P1, P2)
    assert np.array_equal(v, vb) and m == mb, (P1, P2)
    assert np.array_equal(Lbn, np.minimum(Ln, P2) + B), (P1, P2)
    assert Lbn.min() >= B and Lbn.max() <= SENT
    return v, Ln, Lbn


PENALTIES = [(8, 32), (1176, 4704), (1, 2), (1, 4704), (4703, 4704), (5, 6), (1, 32767), (32766, 32767), (100, 32767), (600, 20000)]


@pytest.mark.parametrize("P1,P2", PENALTIES)
def test_planted_states(P1, P2):
    """0, P2 - 1, P2, P2 + 1 and 32767 as a state value at both ends and in the middle, each beside every other; the cost
    such that m is 0 and such that it is 32767 - P2 (the largest a pixel inside the regime can have: v <= C + P2 <= 32767)."""
    vals = sorted({0, 1, max(P2 - 1, 0), P2, min(P2 + 1, SENT), SENT, P1, max(P2 - P1, 0), min(P1 + 1, SENT)})
    n = 0
    for a in vals:
        for b in vals:
            for c in vals:
                L = np.array([a, b, c, 0, c, b, a, 0, b, a], dtype=np.int64)     # (a normalised state has a zero)
                for c0 in (0, SENT - P2):
                    C = np.full(L.size, c0, dtype=np.int64)
                    v, Ln, Lbn = _both(C, L, P1, P2)
                    assert v.min() == c0                                          # m at 0 and at 32767 - P2
                    n += 1
    assert n >= 2 * 27


@pytest.mark.parametrize("P1,P2", PENALTIES)
def test_random_walk_of_states(P1, P2):
    """Many steps in a row from the zero state, each form fed its OWN next state: the biased state stays min(L, P2) + B along
    the whole walk, v and m stay identical.  Costs up to 32767 - P2 keep every v inside int16."""
    rng = np.random.default_rng(P1 * 65537 + P2)
    D = 48
    B = SENT - P2
    L = np.zeros(D, dtype=np.int64)
    Lb = np.full(D, B, dtype=np.int64)                      # the start state of an active lane: splat(B)
    cmax = SENT - P2
    for step in range(200):
        kind = step % 4
        if kind == 0:
            C = rng.integers(0, cmax + 1, D)
        elif kind == 1:
            C = np.minimum(rng.integers(0, 2, D) * cmax, cmax)                    # the extremes only
        elif kind == 2:
            C = np.minimum(np.abs(np.arange(D) - rng.integers(0, D)) * max(P1, 1) + rng.integers(0, 3, D), cmax)
        else:
            C = np.full(D, rng.integers(0, cmax + 1))
        v, m, Ln = plain_step(C, L, P1, P2)
        vb, mb, Lbn = biased_step(C, Lb, P1, P2)
        assert np.array_equal(v, vb) and m == mb, (step, P1, P2)
        assert np.array_equal(Lbn, np.minimum(Ln, P2) + B), (step, P1, P2)
        L, Lb = Ln, Lbn


@pytest.mark.parametrize("NP", [1, 2, 4])
def test_neighbour_minimum_from_one_word_per_register(NP):
    """The biased form builds min(L(d-1), L(d+1)) of a register {L(d_lo), L(d_hi)} from ONE shifted word, w = {high half of
    the previous register, low half of the next one} = {L(d_lo - 1), L(d_hi + 1)}, and the register's own halves swapped
    (the packed minimum's operand selects): {min(L(d_hi), w.lo), min(L(d_lo), w.hi)}.  Registers in lane order, NP per
    lane, the sentinel register beyond both ends of the wave, as the lane shifts bring it in."""
    rng = np.random.default_rng(NP)
    lanes = 6
    L = rng.integers(0, SENT + 1, 2 * NP * lanes)
    regs = L.reshape(-1, 2)                                  # [register][lo, hi]
    sent = np.array([[SENT, SENT]])
    prev = np.concatenate((sent, regs[:-1]))
    nxt = np.concatenate((regs[1:], sent))
    w = np.stack((prev[:, 1], nxt[:, 0]), axis=1)
    nb = np.minimum(regs[:, ::-1], w)
    assert np.array_equal(nb.reshape(-1), _neigh(L))


def test_sentinel_lanes_at_both_ends():
    """Idle lanes of a partial wave hold 32767 in both forms (the kernel puts it there by a select, not by arithmetic): seen
    from the last active disparity it is the sentinel beyond the end -- "P2 or more" -- in the biased domain too."""
    P1, P2 = 7, 50
    B = SENT - P2
    L = np.array([SENT, SENT, 3, 0, 60, 2, SENT, SENT], dtype=np.int64)
    act = slice(2, 6)
    C = np.array([0, 0, 5, 9, 1, 4, 0, 0], dtype=np.int64)
    Lb = np.where(L == SENT, SENT, np.minimum(L, P2) + B)
    t = np.minimum(np.minimum(_sat(_neigh(L) + P1), L), P2)
    tb = np.minimum(_sat(_neigh(Lb) + P1), Lb)
    assert np.array_equal((t + B)[act], tb[act])
    v, vb = (C + t)[act], (C - B + tb)[act]
    assert np.array_equal(v, vb)
    # and with the whole vector active, the ends see the sentinel the shifts bring in
    _both(C[act], L[act], P1, P2)
