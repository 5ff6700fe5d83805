"""k_pix reads its disparity windows from LDS (csrc/kernels_cost.h): the chunk's segment of the six right-image planes is
staged widened to 16 bits in two copies one element apart, behind a per-chunk pad that makes the first column's window
8-byte aligned, and a block of four columns takes its windows as aligned reads.  What can go wrong is addressing: the pad
(four values, from the chunk's length), the last block of a chunk (one to three columns), a chunk shorter than a block, the
zero fill where the segment leaves the image, and each lane packing's read widths.  Every case compares every stage tap
-- C above all -- and the headroom record with the oracle (parity_util.compare_stages), bit for bit, on frames 9 rows high.
(upstream counterpart of what the kernel computes: calcPixelCostBT)"""
import numpy as np
import pytest

import parity_util as U
from oracle import oracle as O
from stereo_reconstruction_cv_amd import _lib, synth
from stereo_reconstruction_cv_amd.stereo import Engine

pytestmark = pytest.mark.gpu

H = 9
STAGES = ("C", "S", "disp_raw", "disp_median", "disp")
PACKINGS = [128, 80, 256, 160, 512, 336]           # NP = 1 full, partial; NP = 2 full, partial; NP = 4 full, partial
REMAINDERS = [0, 1, 2, 3, 4, 5, 6, 7, 126, 127]    # W1 % 128: all four pads, tails of 0..3 columns, a last chunk of 1..3 columns


def _check(W, D, seed, minD=0, bs=5, schedule=1, sweep_rows=0, W1=None):
    l, r, _ = synth.make_pair(H, W, D, seed)
    p = U.params(D, bs, minD, 1, speckleWindowSize=30, speckleRange=2)
    plan = _lib.debug_plan(p, H, W, schedule=schedule, sweep_rows=sweep_rows)
    # the pipeline k_pix belongs to, the wave form of it (not k_pix_px), chained sweeps in throughput mode: read, not assumed
    assert plan["byte_cost"] == 1 and plan["pix_px"] == 0 and plan["chain"] == int(schedule == 2), plan
    assert W1 is None or plan["W1"] == W1, plan
    rep, t, h = U.compare_stages(l, r, p, schedule=schedule, sweep_rows=sweep_rows)
    assert t["headroom"]["ok"], "case left the int16 regime"
    assert set(STAGES) | {"headroom"} <= set(rep), rep
    bad = [U.describe_mismatch(k, h[k], t[k]) for k, n in rep.items() if n]
    assert not bad, f"{(W, D, minD)}: " + "\n".join(bad)
    return h


@pytest.mark.parametrize("rem", REMAINDERS)
@pytest.mark.parametrize("D", PACKINGS)
def test_chunk_remainders(D, rem):
    W1 = 128 + rem if rem else 256                      # W1 >= 129: a full chunk in front of the remainder
    _check(W1 + D, D, 8000 + 10 * D + rem, W1=W1)


@pytest.mark.parametrize("W1", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("D", [96, 256, 512])
def test_narrow_frames(D, W1):
    """a single chunk: shorter than a block, exactly a block, a block and a tail of two"""
    _check(W1 + D, D, 8100 + 10 * D + W1, bs=3, W1=W1)


@pytest.mark.parametrize("minD", [-6, 3])
@pytest.mark.parametrize("D", [128, 256])
def test_disparity_offsets(D, minD):
    """minX1 and the mirrored base of the segment move with minDisparity: the segments of the row's first and last chunk
    end at the image edges (the last one at position 0 for -6).  What lies past the edges is the zero fill, which the
    lanes past D of the partial packings and of D = 48, 64 read"""
    _check(D + 140, D, 8200 + D + minD, minD=minD)


@pytest.mark.parametrize("D", [48, 64])
def test_small_d_with_idle_lanes(D):
    """k_pix<1> with lanes past D: they read their windows like the others and store nowhere"""
    _check(D + 131, D, 8300 + D, W1=131)


def test_throughput_mode_and_the_batch_entry():
    """the form the benchmark runs: schedule 2 with chained sweeps (bands of 4 rows), one pair through every tap and three
    pairs through the batch entry"""
    D, W = 256, 256 + 131
    _check(W, D, 8400, schedule=2, sweep_rows=4, W1=131)
    p = U.params(D, 5, 0, 1, speckleWindowSize=30, speckleRange=2)
    pairs = [synth.make_pair(H, W, D, 8401 + i)[:2] for i in range(3)]
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, 2)
    eng.set_option(_lib.SGM_OPT_SWEEP_ROWS, 4)
    disps, _ = eng.compute_batch_host(np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]), synth.default_Q(W))
    oracle = [O.sgbm_compute(a, b, taps=True, **p) for a, b in pairs]
    for i, (want, _) in enumerate(oracle):
        assert np.array_equal(disps[i], want), (i, int((disps[i] != want).sum()))
    hr = eng.headroom()
    assert hr == dict(ok=all(t["headroom_ok"] for _, t in oracle), max_cost_plus_p2=max(t["max_cost_plus_p2"] for _, t in oracle),
                      max_delta=max(t["max_delta"] for _, t in oracle)), hr
