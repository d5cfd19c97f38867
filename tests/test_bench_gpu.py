"""bench.py's plain run on the GPU: one small `--dump-outputs` run (c2's grid, 3 streams, 1 warm-up + 2 timed
steps).  The line is the plain one (no roofline, CPU baseline, pose check or targets), the dumped arrays are what
the last timed step left, and they equal the CPU oracle's replay of the same seeded scans bit for bit.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import oracle as O
from slam2d import synth

pytestmark = pytest.mark.gpu

B, K, W = 3, 2, 1


def test_plain_run_line_and_dumped_outputs(gpu, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(bench.REPO, "bench.py"), "--gpus", "1", "--config", "c2",
                        "--streams", str(B), "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["metric"] == bench.METRIC and out["unit"] == "scans/s" and out["higher_is_better"] and out["dtype"] == "f32"
    assert out["steps"] == K and out["warmup"] == W and out["full"] is False
    # ms_per_step is the timed region over the K steps, and value the scans of those steps over the same time
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(B / (out["ms_per_step"] * 1e-3), rel=2e-3)
    assert out["roofline"] is None and out["cpu_baseline"] is None and out["pose_vs_ref"] is None
    assert "targets" not in out and "speedup_vs_cpu_1core" not in out
    assert out["config"]["map_updates_per_scan"] == 1.0   # exactly K timed steps, each updating every stream's map

    names = {"pose", "covariance", "map_updated", "updated_cells", "logodds_stream0_level0",
             f"logodds_stream{B - 1}_level0"}
    assert {f[:-4] for f in os.listdir(tmp_path) if f.endswith(".npy")} == names
    got = {n: np.load(tmp_path / f"{n}.npy") for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 10 ** 6
    assert got["pose"].shape == (B, 3) and got["covariance"].shape == (B, 3, 3)
    assert np.array_equal(got["map_updated"], np.ones(B, np.float32))

    # the oracle on the scans the benchmark generates (its seed and generator, so the same ranges in this process
    # as in the benchmark's; the reference's summation order, forced update)
    import torch

    d_rng = torch.empty((K + W, B, synth.N_BEAMS), dtype=torch.float32, device="cuda")
    bench.fill_device_ranges(d_rng, 0, 12345)
    ranges = d_rng.cpu().numpy()
    size = bench.CONFIGS["c2"]["map_size"]
    for s in (0, B - 1):
        h = O.HectorOracle(0.05, size, (0.5, 0.5), 1, reduce_threads=0)
        h.set_update_factors(0.4, 0.9)
        h.set_thresholds(-1.0, -1.0)
        for k in range(K + W):
            pose, _, _ = h.process(synth.ranges_to_points(ranges[k, s].astype(np.float64))[0])
        logodds, _ = h.level(0)
        h.close()
        assert np.array_equal(got["pose"][s].view(np.int32), pose.view(np.int32)), (s, got["pose"][s], pose)
        m = got[f"logodds_stream{s}_level0"]
        assert m.dtype == np.float32 and np.array_equal(m.view(np.int32).reshape(-1), logodds.view(np.int32).reshape(-1))
        assert np.count_nonzero(m) > 1000
