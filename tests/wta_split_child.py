"""Child process of tests/test_gpu_wta_split.py (needs an MI355X): the split winner-take-all on an engine with a history.
One engine runs a larger frame through the separate pass (debug 2048), then -- every buffer poisoned (SGM_OPT_POISON,
csrc/sgm_debug.h), the switch armed so that the raw-record buffer it now allocates is poisoned too -- a smaller frame of
another width through the split form, then the first shape again through the split form.  Every map and the headroom record
must equal the oracle's.  Prints WTA_SPLIT_HISTORY_OK."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402

import parity_util as U  # noqa: E402
from oracle import oracle as O  # noqa: E402
from stereo_reconstruction_cv_amd import _lib, synth  # noqa: E402
from stereo_reconstruction_cv_amd.stereo import Engine  # noqa: E402


def main():
    D = 256
    p = U.params(D, 5, 0, 1, speckleWindowSize=30, speckleRange=2)
    eng = Engine(p)
    eng.set_option(_lib.SGM_OPT_SCHEDULE, 2)
    steps = ((44, 330, 2048, None), (27, 291, 0, 0xFF), (44, 330, 0, 0x7F), (27, 291, 2048, 0x00), (27, 291, 0, 0xA5))
    for k, (H, W, dbg, byte) in enumerate(steps):
        l, r, _ = synth.make_pair(H, W, D, 6100 + H)
        want, t = O.sgbm_compute(l, r, taps=True, **p)
        eng.set_option(_lib.SGM_OPT_DEBUG, dbg)
        if byte is not None:
            eng.set_option(_lib.SGM_OPT_POISON, byte)
        got = eng.compute_host(l, r)
        raw = eng.tap(_lib.SGM_TAP_DISP_RAW, H, W)
        assert np.array_equal(raw, t["disp_raw"]), (k, U.describe_mismatch("disp_raw", raw, np.asarray(t["disp_raw"])))
        assert np.array_equal(got, want), (k, U.describe_mismatch("disp", got, np.asarray(want)))
        assert eng.headroom() == dict(ok=bool(t["headroom_ok"]), max_cost_plus_p2=t["max_cost_plus_p2"], max_delta=t["max_delta"]), k
    eng.set_option(_lib.SGM_OPT_POISON, -1)
    print("WTA_SPLIT_HISTORY_OK", flush=True)


if __name__ == "__main__":
    main()
