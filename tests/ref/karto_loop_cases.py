"""The directed cases and the seeded random graphs of the loop-closure search tests (tests/test_karto_loop_cpu.py,
tests/test_karto_loop_gpu.py, tests/ref/make_karto_loop_golden.py).  Test infrastructure only.

A case is a dict: laser (kt_laser's fields), params (kl_params' fields), ranges [n, n_readings], poses [n, 3], ends
[m, 2] (edges in insertion order, bulk form: no dedupe) and queries [k, 4] = scan, start_num, n_scans, n_edges.
The position cases run with use_scan_barycenter = 0 and one reading per scan, so a scan's reference position is its
pose's x, y exactly and every squared distance can be read off the coordinates.
"""
from __future__ import annotations

import math

import numpy as np

REFERENCE_READINGS = (1, 63, 64, 65, 1081)


def laser(n_readings: int) -> dict:
    return {"minimum_angle": -2.35, "angular_resolution": 4.7 / max(1, n_readings - 1), "minimum_range": 0.1,
            "range_threshold": 12.0, "n_readings": int(n_readings)}


def params(link=1.5, loop=10.0, min_chain=5, bary=1) -> dict:
    return {"link_scan_maximum_distance": float(link), "loop_search_maximum_distance": float(loop),
            "loop_match_minimum_chain_size": int(min_chain), "use_scan_barycenter": int(bary)}


def _case(las, prm, ranges, poses, ends=(), queries=()) -> dict:
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
    return {"laser": las, "params": prm,
            "ranges": np.ascontiguousarray(ranges, np.float64).reshape(len(poses), las["n_readings"]), "poses": poses,
            "ends": np.ascontiguousarray(ends, np.int32).reshape(-1, 2),
            "queries": np.ascontiguousarray(queries, np.int32).reshape(-1, 4)}


def position_case(xy, ends, queries, **prm) -> dict:
    """use_scan_barycenter = 0: the reference positions are xy."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    poses = np.concatenate([xy, np.zeros((len(xy), 1))], axis=1)
    return _case(laser(1), params(bary=0, **prm), np.ones((len(xy), 1)), poses, ends, queries)


def path_edges(n):
    return [(i, i + 1) for i in range(n - 1)]


# --------------------------------------------------------------------------------------------- reference positions
def tree_sensitive_scan(n_readings=1081, seed=5):
    """A full scan far from the origin: its 1081 points' sequential sum and a pairwise sum round differently (asserted
    in tests/test_karto_loop_cpu.py)."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 11.0, n_readings), np.array([100.3, -57.7, 0.4])


def reference_case(n_readings: int, bary=1) -> dict:
    """Seven scans: random, no valid reading, NaN / +-inf among the readings, readings exactly at minimum_range and at
    range_threshold (both valid), every other reading invalid, the tree-sensitive scan's recipe, one valid reading."""
    las = laser(n_readings)
    rng = np.random.default_rng(1000 + n_readings)
    n = n_readings
    r = [rng.uniform(0.2, 11.0, n)]
    r.append(np.where(np.arange(n) % 2 == 0, 0.05, 12.5))
    s = rng.uniform(0.2, 11.0, n)
    s[::3] = np.nan
    s[1::5] = np.inf
    s[2::7] = -np.inf
    r.append(s)
    s = np.full(n, 13.0)
    s[0] = las["minimum_range"]
    s[-1] = las["range_threshold"]
    s[n // 2] = las["range_threshold"] if n > 2 else s[n // 2]
    r.append(s)
    s = rng.uniform(0.2, 11.0, n)
    s[1::2] = 0.0
    r.append(s)
    ts, tpose = tree_sensitive_scan(n, 5)
    r.append(ts)
    s = np.full(n, np.nan)
    s[n - 1] = 3.25
    r.append(s)
    poses = rng.uniform(-3.0, 3.0, (len(r), 3))
    poses[5] = tpose
    return _case(las, params(bary=bary), np.stack(r), poses)


def reference_cases() -> dict:
    out = {f"ref{n}": reference_case(n) for n in REFERENCE_READINGS}
    out["ref65_sensor"] = reference_case(65, bary=0)
    return out


# --------------------------------------------------------------------------------------------- directed searches
def case_threshold() -> dict:
    """link = loop = 4, the query at the origin and its direct neighbour 3 at (4, 0): d2 == 16.0 exactly, in range for
    the chain tests (16 < 16 + 1e-6) but failing the visitor (16 <= 16 - 1e-6 is false): scan 3 is an A and not linked.
    Scan 2 at (3.99999995, 0) has d2 = 15.9999996 > 16 - 1e-6 and fails the visitor too; scan 1 at (3.999, 0) passes.
    The run 2..3 reaches the end of the scans."""
    return position_case([[0, 0], [3.999, 0], [3.99999995, 0], [4, 0]], [(0, 1), (0, 2), (0, 3)],
                         [(0, 0, -1, -1), (0, 3, -1, -1)], link=4.0, loop=4.0, min_chain=1)


def case_through_out_of_range() -> dict:
    """0 - 1 - 2 with 1 out of the visitor's range: 2 is seen by nobody, so it is not linked although it is near."""
    return position_case([[0, 0], [5, 0], [1, 0], [0.5, 0]], [(0, 1), (1, 2), (2, 3)], [(0, 0, -1, -1), (3, 0, -1, -1)],
                         link=1.5, loop=3.0, min_chain=1)


def case_two_parents() -> dict:
    """1 and 2 are expanded in one batch and both push 3 and 4, in opposite orders: the first parent's order (4, 3)
    wins.  adj(1) = 0, 4, 3; adj(2) = 0, 3, 4."""
    xy = [[0, 0], [0.1, 0], [0, 0.1], [0.1, 0.1], [0.2, 0.1], [9, 9]]
    return position_case(xy, [(0, 1), (0, 2), (2, 3), (1, 4), (1, 3), (2, 4), (4, 5)], [(0, 0, -1, -1)], link=1.5,
                         loop=3.0, min_chain=1)


def case_both_directions() -> dict:
    """a -> b, b -> a and the same edge a -> b again (the bulk form does not dedupe): b sits three times in a's list."""
    xy = [[0, 0], [0.3, 0], [0.6, 0], [0.9, 0]]
    return position_case(xy, [(0, 1), (1, 0), (0, 1), (1, 2), (2, 1), (3, 2)], [(0, 0, -1, -1), (2, 0, -1, -1)], link=1.5,
                         loop=3.0, min_chain=1)


def case_star(leaves=100) -> dict:
    """A frontier wider than one batch of 64: the centre has `leaves` neighbours (one lane expands a long adjacency
    list), each with a second-ring neighbour, some of those out of range, added in a scrambled order."""
    xy = [[0.0, 0.0]]
    for i in range(leaves):
        a = 2.0 * math.pi * i / leaves
        xy.append([math.cos(a), math.sin(a)])
    for i in range(leaves):
        a = 2.0 * math.pi * i / leaves
        r = 1.4 if i % 3 else 2.0  # link 1.5: every third one is out of range
        xy.append([r * math.cos(a), r * math.sin(a)])
    ends = [(0, 1 + (i * 37) % leaves) if i % 2 else (1 + (i * 37) % leaves, 0) for i in range(leaves)]
    ends += [(1 + i, 1 + leaves + (i * 13) % leaves) for i in range(leaves)]
    ends += [(1 + leaves + i, 1 + leaves + (i + 1) % leaves) for i in range(0, leaves, 2)]
    return position_case(xy, ends, [(0, 0, -1, -1), (1 + leaves, 0, -1, -1), (7, 3, -1, -1)], link=1.5, loop=1.8,
                         min_chain=2)


def case_loop_runs() -> dict:
    """FindPossibleLoopClosure's exits on one path graph (loop 3, min_chain 10, query 36 at the origin):
    0..9 near (a run of exactly min_chain, ended by the out-of-range scan 10), 10..19 far, 20..24 near (too short),
    25..29 far, 30..34 near but unlinked (34 - 35 is not an edge and 30 hangs off the far scan 29), 35..38 linked to the
    query (35 and 37 directly, 38 through 37): the run 30..34 is followed by a near-linked scan and dropped.  39 far,
    40..41 near and reachable only through 39: a run that reaches the end of the scans, returned at length 2."""
    xs = {}
    for i in range(42):
        near = i < 10 or 20 <= i < 25 or 30 <= i < 39 or i >= 40
        xs[i] = [0.05 * (i - 36), 0.01 * (i % 3)] if near else [20.0 + i, 0.0]
    ends = [e for e in path_edges(42) if e != (34, 35)]
    q = 36
    return position_case([xs[i] for i in range(42)], ends,
                         [(q, 0, -1, -1), (q, 1, -1, -1), (q, 10, -1, -1), (q, 31, -1, -1), (q, 41, -1, -1),
                          (q, 42, -1, -1), (q, 0, 40, -1), (q, 0, 37, 36), (3, 0, -1, -1)],
                         link=1.5, loop=3.0, min_chain=10)


def case_near_chains() -> dict:
    """FindNearChains on a path with two earlier passes near the query 30 (link 1.5, min_chain 4).  The closure edges
    30 -> 16 and 30 -> 6 are added in that order, so the breadth-first order meets the run 15..17 (short: KL_CHAIN_LONG
    clear) before the run 5..8 (long).  6 and 7 are equally near the query: the first minimum, 6, is the closest.  The
    run 27..32 holds the query and is invalid.  20..22 are near but linked to nobody in range: no chain."""
    xy = np.zeros((36, 2))
    xy[:, 0] = 30.0 + np.arange(36)  # far, apart from each other
    xy[30] = [0.0, 0.0]
    for i, x in zip((27, 28, 29, 31, 32), (-0.9, -0.6, -0.3, 0.3, 0.6)):
        xy[i] = [x, 0.0]
    xy[5], xy[6], xy[7], xy[8] = [-0.5, 1.0], [-0.25, 0.5], [0.25, 0.5], [0.5, 1.0]
    xy[15], xy[16], xy[17] = [-0.4, -0.8], [0.0, -0.7], [0.4, -0.8]
    xy[20], xy[21], xy[22] = [1.0, 0.2], [1.0, 0.0], [1.0, -0.2]
    ends = path_edges(31) + [(30, 16), (30, 6)] + [(i, i + 1) for i in range(31, 35)] + [(30, 31)]
    return position_case(xy, ends, [(30, 0, -1, -1), (30, 0, 31, 32), (30, 0, 31, 31), (30, 0, 31, 30), (16, 0, -1, -1),
                                    (6, 4, 20, 19), (35, 0, -1, -1)], link=1.5, loop=2.5, min_chain=4)


def noisy_circle(rng, n, radius, laps=2.0, n_readings=17, noise=0.05, extra_edges=0):
    """A looping trajectory with scans: `laps` turns of a circle, path edges and random extra edges."""
    a = 2.0 * math.pi * laps * np.arange(n) / max(1, n - 1)
    poses = np.stack([radius * np.cos(a) + rng.normal(0, noise, n), radius * np.sin(a) + rng.normal(0, noise, n),
                      a + math.pi / 2.0 + rng.normal(0, 0.05, n)], axis=1)
    ranges = rng.uniform(0.05, 13.0, (n, n_readings))
    ends = path_edges(n)
    for _ in range(extra_edges):
        s, t = rng.integers(0, n, 2)
        if s != t:
            ends.append((int(s), int(t)))
    return ranges, poses, ends


def case_circle_scans(n=90, seed=3) -> dict:
    """Barycentres from real readings on a two-lap circle, the node's parameters scaled to the circle."""
    rng = np.random.default_rng(seed)
    ranges, poses, ends = noisy_circle(rng, n, 2.0, extra_edges=6)
    queries = [(n - 1, 0, -1, -1), (n // 2, 0, n // 2 + 1, n // 2), (n - 5, 7, n - 2, -1), (3, 0, -1, -1)]
    return _case(laser(17), params(link=0.8, loop=1.6, min_chain=3), ranges, poses, ends, queries)


def search_cases() -> dict:
    return {"threshold": case_threshold(), "through_out_of_range": case_through_out_of_range(),
            "two_parents": case_two_parents(), "both_directions": case_both_directions(), "star": case_star(),
            "loop_runs": case_loop_runs(), "near_chains": case_near_chains(), "circle_scans": case_circle_scans()}


def directed_cases() -> dict:
    out = reference_cases()
    out.update(search_cases())
    return out


# --------------------------------------------------------------------------------------------- the random sweep
def random_case(seed: int) -> dict:
    """A graph of 2 .. 120 scans: a random walk or a noisy circle, random extra edges, one query with a random scan
    and start_num (position form: the sweep is about the lists, the barycentres have their own cases)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 121))
    if rng.random() < 0.5:
        step = rng.normal(0.0, 0.35, (n, 2))
        xy = np.cumsum(step, axis=0)
    else:
        laps = rng.uniform(1.0, 3.0)
        a = 2.0 * math.pi * laps * np.arange(n) / n
        rad = rng.uniform(0.5, 3.0)
        xy = np.stack([rad * np.cos(a), rad * np.sin(a)], axis=1) + rng.normal(0.0, 0.1, (n, 2))
    ends = [e for e in path_edges(n) if rng.random() < 0.93]
    for _ in range(int(rng.integers(0, 6))):
        s, t = rng.integers(0, n, 2)
        if s != t:
            ends.append((int(s), int(t)))
    scan = int(rng.integers(0, n))
    start = int(rng.integers(0, n + 1)) if rng.random() < 0.5 else 0
    prefix = rng.random() < 0.2
    ns = int(rng.integers(scan + 1, n + 1)) if prefix else -1
    ne = int(rng.integers(0, len(ends) + 1)) if prefix else -1
    return position_case(xy, ends, [(scan, start, ns, ne)], link=float(rng.uniform(0.4, 1.5)),
                         loop=float(rng.uniform(0.8, 3.0)), min_chain=int(rng.integers(1, 8)))
