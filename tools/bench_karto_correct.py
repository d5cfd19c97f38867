#!/usr/bin/env python3
"""Times one CorrectPoses round and one per-scan refresh round of a Karto fleet through the host-indexed path and
through the record-indexed kc_ path, in one process and binary.

    python tools/bench_karto_correct.py [--graphs 64 1024] [--scans 64 1024 4096] [--readings 1081] [--reps 7]
                                        [--warm 3] [--max-gib 48] [--out bench_outputs/karto_correct_bench.json]

A fleet is G graphs of S scans each (chains with one closure constraint that disagrees with the poses, so the optimiser
has work), a LoopSearchFleet, a SpaFleet and ONE ScanMatcher pool per path (the loop matcher would double the same
kernel's time), and one scan pool of G * S scans that both paths read.  Every eighth graph closes a loop.
  refresh round   every graph's newest scan got a new pose (the sequential match, AddEdges' weighted mean):
    host    per graph kl_set_scans_device + kt_set_scans_device with host integers graph, first, count;
    device  kc_refresh_jobs_device on G device-resident job records.
  correct round   CorrectPoses for the closing graphs:
    host    per closing graph spa_compute_device, spa_device_poses (which is where a device-edited graph would be
            pulled back; these graphs are host-built, so the call here only returns the pointer), a device-to-device
            copy of the poses into the pool, kl_set_scans_device and kt_set_scans_device over the graph's scans;
    device  kc_correct_poses_device on the G job and closure records.
The optimiser runs `--niter` LM iterations of at most `--cg` PCG iterations in both paths (the same kernel; its time is
not what this tool is about).  Each round is timed by the host clock from the first call to a device synchronise; the two
paths alternate; median and minimum over `reps` rounds after `warm` rounds.  One more round per path reads the stages'
kernel timers.  The refresh kernels' ranges bytes over their time are set against the HBM peak of 8 TB/s
(MI355X_MICROARCH.md), beside the sine / cosine pairs per second, to say which of the two bounds each.  After the last
round the pool poses and kl_get_reference of the first and the last graph are compared byte for byte between the
paths.  A cell whose matcher pools would not fit `--max-gib` is skipped and listed as such.  There is no pass / fail
threshold.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "creating-2d-laser-slam-from-scratch_amd", "python")]

HBM_PEAK = 8.0e12
PREC = np.array([[120.0, 3.0, -2.0], [3.0, 90.0, 1.5], [-2.0, 1.5, 400.0]])
POOL_BYTES_PER_READING = 8 + 16 + 16 + 1 + 8   # a matcher pool: ranges, points, local points, bad, events


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--scans", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--readings", type=int, default=1081)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--niter", type=int, default=2)
    ap.add_argument("--cg", type=int, default=10)
    ap.add_argument("--max-gib", type=float, default=48.0)
    ap.add_argument("--out", default=os.path.join(REPO, "bench_outputs", "karto_correct_bench.json"))
    a = ap.parse_args()

    import torch

    from slam2d import karto as kt
    from slam2d import karto_correct as kc
    from slam2d import karto_link as ke
    from slam2d import karto_loop as kl
    from slam2d import spa as sp

    assert torch.cuda.is_available(), "bench_karto_correct needs a HIP device"
    n = a.readings
    laser = kt.laser(n, -2.35, 4.7 / max(n - 1, 1), 0.1, 12.0)
    prm = kl.default_params(link_scan_maximum_distance=1.5, loop_search_maximum_distance=4.0,
                            loop_match_minimum_chain_size=3, use_scan_barycenter=1)
    spa_prm = sp.default_params(niter=a.niter, max_cg_iters=a.cg)

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    D2D = 3
    rows_out, skipped = [], []
    for G in a.graphs:
        for S in a.scans:
            need = 2.0 * G * S * n * POOL_BYTES_PER_READING + 8.0 * G * S * n
            if need > a.max_gib * 2**30:
                skipped.append({"graphs": G, "scans": S, "reason": f"the two matcher pools and the scan pool need {need / 2**30:.0f} GiB"})
                print(f"graphs {G:5d} scans {S:5d} | skipped: {skipped[-1]['reason']}")
                continue
            P = G * S
            closing = np.arange(G) % 8 == 0
            rng = np.random.default_rng(3)
            d_ranges = torch.empty((P, n), dtype=torch.float64, device="cuda").uniform_(0.5, 11.0)
            k = np.arange(S)
            poses = np.stack([0.4 * k, 0.05 * np.sin(0.3 * k), 0.02 * np.sin(0.1 * k)], axis=1)
            ends = np.concatenate([np.stack([np.arange(1, S), np.arange(0, S - 1)], axis=1), [[S - 1, 0]]]).astype(np.int32)
            rel = poses[:-1] - poses[1:]
            means = np.concatenate([rel, [[-0.4 * (S - 1) + 0.3, 0.1, 0.01]]])   # the closure disagrees with the chain
            precs = np.tile(PREC.reshape(9), (S, 1))
            fleets = {}
            for path in ("host", "device"):
                f = kl.LoopSearchFleet(laser, prm, G, S, S + 8, 1)
                s = sp.SpaFleet(G, S, S + 8)
                m = kt.ScanMatcher(laser, kt.default_params(), max_matches=1, max_scans=P, max_base=1)
                d_pool = torch.from_numpy(np.tile(poses, (G, 1))).cuda()
                for g in range(G):
                    f.set_pool_offset(g, g * S)
                    f.set_graph(g, S, ends[:-1])
                    s.set_graph(g, np.arange(S, dtype=np.int32), poses, ends, means, precs)
                s.compute(0, G, sp.default_params(niter=0))   # uploads every graph
                f.search([(0, 0, 0, -1, -1)])                 # likewise
                torch.cuda.synchronize()
                for g in range(G):
                    f.set_scans_device(g, 0, S, d_ranges[g * S:].data_ptr(), d_pool[g * S:].data_ptr())
                m.set_scans_device(0, P, d_ranges.data_ptr(), d_pool.data_ptr())
                fleets[path] = (f, s, m, d_pool)
            stage = kc.PoseCorrection(G, S, None, max(G, 1))
            jobs = ke.jobs([(g, S - 1, g * S, S - 2, g, -1, 0, 0) for g in range(G)])
            cl = np.zeros(G, ke.CLOSURE_DTYPE)
            cl["chain"] = np.where(closing, 0, -1)
            d_jobs, d_cl = dev(jobs), dev(cl)
            stream = torch.cuda.Stream()   # one stream of the caller's for every context of a path
            st = stream.cuda_stream
            torch.cuda.synchronize()

            def move(d_pool, r):   # the newest scans' new poses: on the device, before the clock starts
                d_pool[S - 1::S, 0] += 0.001 * (r + 1)

            def host_refresh():
                f, s, m, d_pool = fleets["host"]
                for g in range(G):
                    o = g * S + S - 1
                    f.set_scans_device(g, S - 1, 1, d_ranges[o:].data_ptr(), d_pool[o:].data_ptr(), st)
                    m.set_scans_device(o, 1, d_ranges[o:].data_ptr(), d_pool[o:].data_ptr(), st)

            def device_refresh():
                f, s, m, d_pool = fleets["device"]
                stage.refresh_jobs_device(d_jobs.data_ptr(), 0, G, d_ranges.data_ptr(), d_pool.data_ptr(), P, f, m, None, st)

            def host_correct():
                f, s, m, d_pool = fleets["host"]
                for g in np.nonzero(closing)[0].tolist():
                    o = g * S
                    s.compute_device(g, 1, spa_prm, st)
                    ptr, cnt = s.device_poses(g)
                    assert hip.hipMemcpyAsync(d_pool[o:].data_ptr(), ptr, 24 * cnt, D2D, st) == 0
                    f.set_scans_device(g, 0, cnt, d_ranges[o:].data_ptr(), d_pool[o:].data_ptr(), st)
                    m.set_scans_device(o, cnt, d_ranges[o:].data_ptr(), d_pool[o:].data_ptr(), st)

            def device_correct():
                f, s, m, d_pool = fleets["device"]
                stage.correct_poses_device(d_jobs.data_ptr(), d_cl.data_ptr(), G, s, d_ranges.data_ptr(), d_pool.data_ptr(), P,
                                           spa_prm, f, m, None, st)

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            times = {k_: [] for k_ in ("host_refresh", "device_refresh", "host_correct", "device_correct")}
            for r in range(a.warm + a.reps):
                for path in ("host", "device"):
                    move(fleets[path][3], r)
                order = (("host_refresh", host_refresh), ("device_refresh", device_refresh), ("host_correct", host_correct),
                         ("device_correct", device_correct))
                for name, fn in (order if r % 2 == 0 else (order[1], order[0], order[3], order[2])):
                    t = timed(fn)
                    if r >= a.warm:
                        times[name].append(t)
            # one further round with the stages' timers on
            kernels = {}
            for path, fns in (("host", (host_refresh, host_correct)), ("device", (device_refresh, device_correct))):
                f, s, m, d_pool = fleets[path]
                move(d_pool, a.warm + a.reps)
                for c in (f, m, stage):
                    c.set_timing(True)
                torch.cuda.synchronize()
                for which, fn in zip(("refresh", "correct"), fns):
                    fn()
                    torch.cuda.synchronize()
                    kv = {}
                    for c in (f, m, stage):
                        kv.update({k_: v for k_, v in c.kernel_times(reset=True).items() if v[1]})
                    kernels[f"{path}_{which}"] = {k_: {"ms": v[0], "launches": v[1]} for k_, v in kv.items()}
                for c in (f, m, stage):
                    c.set_timing(False)
            for g in (0, G - 1):
                x = [fleets[p][3][g * S:(g + 1) * S].cpu().numpy().tobytes() for p in ("host", "device")]
                assert x[0] == x[1], f"graph {g}: the pool poses differ between the paths"
                y = [fleets[p][0].get_reference(g, 0, S).tobytes() for p in ("host", "device")]
                assert y[0] == y[1], f"graph {g}: the reference positions differ between the paths"
            scans_corrected = int(closing.sum()) * S
            bound = {}
            for name in ("kl_refresh_kernel", "kt_refresh_kernel"):
                ms = kernels["device_correct"].get(name, {}).get("ms", 0.0)
                if ms > 0:
                    bytes_s = scans_corrected * n * 8 / (ms * 1e-3)
                    bound[name] = {"ms": ms, "ranges_bytes_per_s": bytes_s, "of_hbm_peak": bytes_s / HBM_PEAK,
                                   "sincos_pairs_per_s": scans_corrected * n / (ms * 1e-3)}
            row = {"graphs": G, "scans": S, "readings": n, "closing": int(closing.sum()), "reps": a.reps, "warm": a.warm,
                   **{f"{k_}_ms_median": statistics.median(v) for k_, v in times.items()},
                   **{f"{k_}_ms_min": min(v) for k_, v in times.items()}, "kernels": kernels, "refresh_kernels_in_correct": bound}
            row["refresh_host_over_device"] = row["host_refresh_ms_median"] / row["device_refresh_ms_median"]
            row["correct_host_over_device"] = row["host_correct_ms_median"] / row["device_correct_ms_median"]
            rows_out.append(row)
            print(f"graphs {G:5d} scans {S:5d} | refresh host {row['host_refresh_ms_median']:.3f} ms device "
                  f"{row['device_refresh_ms_median']:.3f} ms (x{row['refresh_host_over_device']:.1f}) | correct host "
                  f"{row['host_correct_ms_median']:.3f} ms device {row['device_correct_ms_median']:.3f} ms "
                  f"(x{row['correct_host_over_device']:.1f})")
            for k_, kv in kernels.items():
                print(f"    {k_}: " + ", ".join(f"{kn} {v['ms']:.3f} ms / {v['launches']}" for kn, v in kv.items()))
            for k_, v in bound.items():
                print(f"    {k_} in the correct round: {v['ranges_bytes_per_s'] / 1e9:.1f} GB/s of ranges "
                      f"({100 * v['of_hbm_peak']:.2f} % of the HBM peak), {v['sincos_pairs_per_s'] / 1e9:.2f} G sin/cos pairs per s")
            sys.stdout.flush()
            stage.close()
            for f, s, m, _ in fleets.values():
                f.close()
                s.close()
                m.close()
            del fleets, d_ranges
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"tool": "bench_karto_correct", "device": torch.cuda.get_device_name(0), "rows": rows_out,
                   "skipped": skipped}, fh, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
