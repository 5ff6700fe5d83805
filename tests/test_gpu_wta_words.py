"""The reducing sweep that stores lane words, on the GPU: the best disparity at every position inside a lane and next to a
lane boundary.  right = left shifted by s columns makes s the best disparity of most matched pixels; s = 1 .. 8 walks the
positions of the first lanes (a lane holds 2 or 4 disparities), the last shifts those of the last lanes, whose neighbour
words come from the lane below / above or are clamped at D - 1.  Every case is tests/test_gpu_wta_split.py's check: the split
form and debug 2048 each equal the oracle in every pixel of the raw map, the final map and the headroom record."""
import numpy as np
import pytest

from stereo_reconstruction_cv_amd import synth
from test_gpu_wta_split import _check_split, _params

pytestmark = pytest.mark.gpu

H = 14          # bands of 12 + 2 rows
GROUPS = {
    (256, "first_lanes"): range(1, 9),
    (256, "last_lanes"): range(247, 255),
    (128, "first_lanes"): range(1, 9),
    (128, "last_lanes"): range(119, 127),
}


@pytest.mark.parametrize("D,group", sorted(GROUPS))
def test_best_at_every_position_of_a_lane(D, group):
    W = D + 44
    left = synth.make_pair(H, W, D, 77)[0]
    for s in GROUPS[(D, group)]:
        right = np.zeros_like(left)
        right[:, :W - s] = left[:, s:]
        want = _check_split(("words", D, s), left, right, _params(D))
        raw = np.asarray(want["disp_raw"])[:, D:]
        share = float((raw == 16 * s).mean())
        print(f"D = {D}, shift {s}: {share:.2f} of the matched columns at 16 s")
        assert share > 0.5, (D, s, share)      # (the oracle alone: 0.79 .. 0.86 for every one of these cases)
