#!/usr/bin/env python3
"""Throughput of the on-device lidar undistortion (ud_correct_batch_device) beside the plain scan ingest
(hs_ingest_batch_device) on the same fleet: what de-skewing costs over treating the sweep as instantaneous.

    python tools/bench_undistort.py [--streams 4608] [--beams 1081] [--imu 24] [--out profiles/undistort_bench.json]

Every input is generated on the device (ranges, the 200 Hz IMU windows, the odometry pairs); both kernels are
timed with HIP events on one stream: after a warm-up, `--reps` windows of `--launches` back-to-back launches each,
the two entry points alternating window by window; the figure of record is the median window.  Bytes per launch
are counted from the shapes: 4 B range in, 12 B cloud point and 8 B container point out per beam (24 B), plus
each scan's window (32 B per IMU sample, 112 B odometry pair, 16 B scan times, 4 B count) and its 16 B of
count / origo / status out.  The plain ingest moves 4 B in and 8 B out per beam.

The measurement runs in a child process under the tool's own time limit (--limit seconds); without a HIP
device it fails.  One JSON line is printed (and written to --out when given).
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "creating-2d-laser-slam-from-scratch_amd", "python"))


def measure(a) -> dict:
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_undistort: no HIP device")
    from slam2d import _lib
    from slam2d.hector import HectorFleet, HsLaser
    from slam2d.undistort import UndistortFleet, default_laser

    B, N, K = a.streams, a.beams, a.imu
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    amin, ainc = -3.0 * np.pi / 4.0, float(np.float32(1.5 * np.pi / (N - 1)))
    tinc = float(np.float32(0.1 / N))
    # device-side inputs
    ranges = torch.rand((B, N), generator=g, device=dev, dtype=torch.float32) * 18.0 + 0.5
    t0 = 100.0 + torch.rand((B,), generator=g, device=dev, dtype=torch.float64)
    scan_time = torch.stack([t0, torch.full_like(t0, tinc)], dim=1).contiguous()
    # IMU at 200 Hz: the first sample 4 ms before the scan start, the last after its end
    if K < 2 or -0.004 + 0.005 * (K - 1) < tinc * (N - 1):
        raise SystemExit("bench_undistort: --imu samples at 200 Hz must cover the 0.1 s sweep (>= 22)")
    ti = t0[:, None] - 0.004 + 0.005 * torch.arange(K, device=dev, dtype=torch.float64)[None, :]
    w = (torch.rand((B, K, 3), generator=g, device=dev, dtype=torch.float64) - 0.5) * 1.0
    imu = torch.cat([ti[:, :, None], w], dim=2).contiguous()
    imu_n = torch.full((B,), K, device=dev, dtype=torch.int32)
    o0 = torch.cat([(t0 - 0.01)[:, None], (torch.rand((B, 6), generator=g, device=dev, dtype=torch.float64) - 0.5)], 1)
    o1 = o0 + torch.tensor([0.09, 0.05, 0.02, 0.0, 0.001, 0.001, 0.03], device=dev, dtype=torch.float64)[None, :]
    odom = torch.stack([o0, o1], dim=1).contiguous()
    cloud = torch.zeros((B, N, 3), device=dev, dtype=torch.float32)
    xy = torch.zeros((B, N, 2), device=dev, dtype=torch.float32)
    n_out = torch.zeros((B,), device=dev, dtype=torch.int32)
    origo = torch.zeros((B, 2), device=dev, dtype=torch.float32)
    status = torch.zeros((B,), device=dev, dtype=torch.int32)
    xy2 = torch.zeros((B, N, 2), device=dev, dtype=torch.float32)
    n2 = torch.zeros((B,), device=dev, dtype=torch.int32)

    uf = UndistortFleet(B, N, K)
    uf.set_scan_geometry(amin, ainc, 0.1, 30.0)
    hf = HectorFleet(B, 0.05, 256, (0.5, 0.5), 1, max_points=N)  # small maps: only the ingest is timed
    uf.set_container_rules(default_laser(N, amin, ainc), hf.scale_to_map())
    hf.set_laser(HsLaser.defaults(N, amin, ainc))
    st = torch.cuda.Stream()
    hs = st.cuda_stream
    torch.cuda.synchronize()

    def run_ud():
        uf.correct_device(B, ranges, N, scan_time, imu, K, imu_n, odom, cloud, N, xy, N, n_out, origo, status,
                          hip_stream=hs)

    def run_ingest():
        hf.ingest_device(B, ranges.data_ptr(), N, xy2.data_ptr(), N, n2.data_ptr(), hip_stream=hs)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            e0.record(st)
            for _ in range(a.launches):
                fn()
            e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.launches  # us per launch

    for _ in range(a.warmup):
        run_ud()
        run_ingest()
    st.synchronize()
    assert int(status.max().item()) == 0 and int(n_out.min().item()) > 0, "the bench inputs must all be corrected"
    ud_us, in_us = [], []
    for _ in range(a.reps):  # alternate the two, window by window
        ud_us.append(window(run_ud))
        in_us.append(window(run_ingest))
    ud_med, in_med = float(np.median(ud_us)), float(np.median(in_us))
    ud_bytes = B * (N * 24 + K * 32 + 112 + 16 + 4 + 16)
    in_bytes = B * (N * 12 + 12)
    res = {"tool": "bench_undistort", "device": torch.cuda.get_device_name(0), "streams": B, "beams": N, "imu_samples": K,
           "warmup": a.warmup, "reps": a.reps, "launches_per_window": a.launches,
           "kernel_src": _lib.source_id_of_library(),
           "undistort": {"us_per_launch_median": ud_med, "us_per_launch_min": float(min(ud_us)),
                         "us_per_launch_max": float(max(ud_us)), "scans_per_s": B / (ud_med * 1e-6),
                         "bytes_per_launch": ud_bytes, "GB_per_s": ud_bytes / (ud_med * 1e-6) / 1e9,
                         "mean_points": float(n_out.float().mean().item())},
           "ingest": {"us_per_launch_median": in_med, "us_per_launch_min": float(min(in_us)),
                      "us_per_launch_max": float(max(in_us)), "scans_per_s": B / (in_med * 1e-6),
                      "bytes_per_launch": in_bytes, "GB_per_s": in_bytes / (in_med * 1e-6) / 1e9,
                      "mean_points": float(n2.float().mean().item())},
           "undistort_over_ingest": ud_med / in_med}
    uf.close()
    hf.close()
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--streams", type=int, default=4608)
    p.add_argument("--beams", type=int, default=1081)
    p.add_argument("--imu", type=int, default=24, help="IMU samples per window (200 Hz)")
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--reps", type=int, default=21)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--limit", type=float, default=240.0, help="time limit of the GPU step, seconds")
    p.add_argument("--out", default="")
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a)))
        return 0
    # the GPU step runs in a fresh child process under this tool's own time limit
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    except subprocess.TimeoutExpired:
        print(f"bench_undistort: the GPU step exceeded its {a.limit:.0f} s limit", file=sys.stderr)
        return 124
    line = next((ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout + r.stderr)
        return r.returncode or 1
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
