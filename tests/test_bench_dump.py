"""bench.py --dump-outputs DIR: after the timed steps the results of the last one go to DIR/<name>.npy (float32 arrays
[pairs, n(, C)] at the n pixel positions of DIR/sample_pixels.npy), at most 64 MB in all and every value finite, so
that two builds can be compared output for output.  The plumbing runs here with the stand-in engine (BENCH_MOCK=1); on an MI355X the dumped
maps, float maps and XYZ images of the real engine must equal the oracle's for the bench's own input pairs."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out, *args, mock=True):
    env = dict(os.environ, **({"BENCH_MOCK": "1"} if mock else {}))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT") + (() if mock else ("BENCH_MOCK",)):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args, "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    a = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(out, "*.npy"))}
    assert all(x.dtype in (np.float32, np.float64) and np.isfinite(x).all() for x in a.values()), \
        [k for k, x in a.items() if not np.isfinite(x).all()]
    return json.loads(lines[0]), a


def _size(out):
    return sum(os.path.getsize(f) for f in glob.glob(os.path.join(out, "*.npy")))


def test_small_outputs_are_written_whole(tmp_path):
    d, a = _bench(tmp_path, "--workload", "tiny", "--steps", "3", "--warmup", "1")
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    H, W, ppg = 96, 480, 2
    assert set(a) == {"sample_pixels", "disparity", "disparity_float", "xyz", "xyz_finite"}
    assert np.array_equal(a["sample_pixels"], np.arange(H * W))
    assert a["disparity"].shape == a["disparity_float"].shape == (ppg, H * W)
    assert a["xyz"].shape == a["xyz_finite"].shape == (ppg, H * W, 3)


def test_non_finite_values_are_written_as_zero_beside_a_mask(tmp_path):
    """the XYZ of a pixel at infinity is inf or NaN: the dump writes 0 there and says so in <name>_finite.npy; a field not
    expected to hold such values refuses to be written with them"""
    import torch

    import bench
    xyz = torch.tensor([[1.0, 2.0, 3.0], [float("inf"), float("-inf"), float("nan")], [4.0, 5.0, 6.0]])
    bench.dump_outputs(str(tmp_path), 3, {"disparity": [torch.tensor([16, -16, 32], dtype=torch.int16)], "xyz": [xyz]},
                       masked=("xyz",))
    got, fin = np.load(tmp_path / "xyz.npy"), np.load(tmp_path / "xyz_finite.npy")
    assert got.dtype == fin.dtype == np.float32 and np.isfinite(got).all()
    assert np.array_equal(got, [[[1, 2, 3], [0, 0, 0], [4, 5, 6]]]) and np.array_equal(fin, [[[1, 1, 1], [0, 0, 0], [1, 1, 1]]])
    assert np.array_equal(np.load(tmp_path / "disparity.npy"), [[16, -16, 32]])
    with pytest.raises(RuntimeError, match="non-finite"):
        bench.dump_outputs(str(tmp_path / "b"), 3, {"xyz": [xyz]})


def test_large_outputs_keep_a_fixed_sample_under_64_mb(tmp_path):
    """one 4K pair with reprojection is 232 MB of results: the dump keeps the same seeded pixel sample run after run"""
    _, a = _bench(tmp_path / "a", "--workload", "c3c5", "--steps", "1", "--warmup", "0")
    _, b = _bench(tmp_path / "b", "--workload", "c3c5", "--steps", "1", "--warmup", "0")
    assert _size(tmp_path / "a") <= 64 * 10 ** 6
    idx = a["sample_pixels"]
    assert 10 ** 5 < len(idx) < 2160 * 3840 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 2160 * 3840
    assert np.array_equal(idx, b["sample_pixels"])
    assert a["xyz"].shape == (1, len(idx), 3) and a["xyz"].dtype == np.float32


def test_rank0_ingest_dumps_the_gathered_point_lists(tmp_path):
    """--ingest rank0 --xyz compact: rank 0 receives the maps and one list of valid points per frame (0 past its count)"""
    _, a = _bench(tmp_path, "--gpus", "2", "--workload", "tinyt", "--ingest", "rank0", "--xyz", "compact", "--steps", "2",
                  "--warmup", "1")
    assert set(a) == {"sample_pixels", "disparity", "points", "point_counts"}
    n = 6
    assert a["disparity"].shape == (n, 96 * 480) and a["points"].shape == (n, 96 * 480, 3) and a["point_counts"].shape == (n,)
    for i, c in enumerate(a["point_counts"].astype(int)):
        assert 0 < c < 96 * 480 and not a["points"][i, c:].any()


def test_steps_must_be_positive(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       env=dict(os.environ, BENCH_MOCK="1"), timeout=300)
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["tiny", "tinyt"])
def test_dumped_outputs_are_what_the_oracle_computes(tmp_path, workload):
    """the real engine, per-pair engines (tiny) and the batch entry in throughput mode (tinyt): every dumped value equals
    the oracle's for the bench's own pairs (seeds 1234 + i)"""
    import bench
    from oracle import oracle as O
    from stereo_reconstruction_cv_amd import synth
    H, W, D, bs, mode, ppg, with_xyz, _, _, _ = bench.WORKLOADS[workload]
    _, a = _bench(tmp_path, "--workload", workload, "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-latency-mode",
                  mock=False)
    assert with_xyz and np.array_equal(a["sample_pixels"], np.arange(H * W))
    Q = synth.default_Q(W)
    for i in range(ppg):
        left, right, _ = synth.make_pair(H, W, D, seed=1234 + i)
        want = O.sgbm_compute(left, right, **bench.sgbm_params(D, bs, mode))
        wf = O.disp_to_float(want)
        wxyz = O.reproject(wf, Q)
        assert np.array_equal(a["disparity"][i], want.reshape(-1).astype(np.float32)), f"pair {i}: maps differ"
        assert np.array_equal(a["disparity_float"][i], wf.reshape(-1))
        fin = np.isfinite(wxyz.reshape(-1, 3))
        assert np.array_equal(a["xyz_finite"][i], fin.astype(np.float32))
        assert np.array_equal(a["xyz"][i][fin], wxyz.reshape(-1, 3)[fin]) and not a["xyz"][i][~fin].any()
