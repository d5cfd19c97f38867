"""Worlds for the Karto scan-intake stage (include/slam2d/karto_process.h): the directed cases of the gate, the odometry
carry, the running-scan trim and the refusals, mixed fleets for the launch shapes, and `step`, one intake -> apply ->
advance round through an implementation (the restatement karto_process_ref, the transcription karto_process_plain, or
a GPU adapter with the same three functions).  Test infrastructure: nothing here is imported by the package.

A world is described in karto_process_ref.py.  Pool rows that hold no scan are POISON bytes, so a row a call writes
without cause shows.  A world may carry "seq": the sequential matcher's kt_result rows, by seq index.
"""
from __future__ import annotations

import math

import numpy as np

import karto_process_ref as R

GAP = 1  # pool slots between two graphs' ranges of slots: a write past a graph's end lands there


def up(v, k=1):
    for _ in range(abs(k)):
        v = float(np.nextafter(v, math.inf if k > 0 else -math.inf))
    return v


def solve_d2(target: float):
    """(dx, dy) whose dx * dx + dy * dy, evaluated in double, is `target` exactly."""
    for frac in (1.0, 0.9, 0.75, 0.6, 0.5):
        dx0 = math.sqrt(target * frac)
        for k in range(-8, 9):
            dx = up(dx0, k)
            rest = target - dx * dx
            if rest < 0.0:
                continue
            dy0 = math.sqrt(rest)
            for j in range(-8, 9):
                dy = up(dy0, j) if dy0 > 0.0 else 0.0
                if dx * dx + dy * dy == target:
                    return dx, dy
    raise AssertionError(f"no exact squared distance for {target!r}")


def results(means, responses=None, statuses=None, seed=0) -> np.ndarray:
    """kt_result rows: the means given, SPD covariances, status KT_OK unless given."""
    m = np.asarray(means, np.float64).reshape(-1, 3)
    rng = np.random.default_rng(7000 + seed)
    r = np.zeros(len(m), R.KT_RESULT)
    r["mean"] = m
    for k in range(len(m)):
        a = rng.normal(size=(3, 3))
        r["covariance"][k] = (0.003 * (a @ a.T + 3.0 * np.eye(3))).reshape(9)
    r["response"] = 0.9 if responses is None else responses
    r["status"] = 0 if statuses is None else statuses
    return r


def build_world(graphs, cands, params=None, n_readings=8, max_scans=16, pool_scans=None, seed=0, g_first=0, seq=None):
    """graphs: per graph a dict(poses [n, 3] = the scans' pool poses, run = (begin, length) (default: the last
    min(n, scan_buffer_size) scans), last_time (default 0), last_odom (default: the last pool pose)).
    cands: per graph of [g_first, g_first + len(cands)) a (row, time, odom): row None takes the next free row of
    ranges_f32, -1 is absent."""
    p = dict(R.DEFAULT_PARAMS)
    p.update(params or {})
    rng = np.random.default_rng(1000 + seed)
    G = len(graphs)
    offsets = np.array([g * (max_scans + GAP) for g in range(G)], np.int32)
    P_ = G * (max_scans + GAP) if pool_scans is None else pool_scans
    pool_poses, pool_ranges = R.poisoned((P_, 3), np.float64), R.poisoned((P_, n_readings), np.float64)
    states = np.zeros(G, R.STATE)
    for g, spec in enumerate(graphs):
        poses = np.asarray(spec.get("poses", np.zeros((0, 3))), np.float64).reshape(-1, 3)
        n = len(poses)
        lo, hi = int(offsets[g]), min(int(offsets[g]) + n, P_)
        if hi > lo:
            pool_poses[lo:hi] = poses[:hi - lo]
            pool_ranges[lo:hi] = rng.uniform(0.05, 12.0, (hi - lo, n_readings))
        length = min(n, int(p["scan_buffer_size"]))
        begin, length = spec.get("run", (n - length, length))
        last_odom = spec.get("last_odom", poses[-1] if n else (0.0, 0.0, 0.0))
        states[g] = R.state(n, begin, length, spec.get("last_time", 0.0) if n else 0.0, last_odom)  # no scans: all zero
    rows, next_row = [], 0
    for row, _, _ in cands:
        if row is None:
            row, next_row = next_row, next_row + 1
        rows.append(row)
    ranges = rng.uniform(0.05, 30.0, (next_row + 1, n_readings)).astype(np.float32)
    ranges[rng.random(ranges.shape) < 0.1] = np.inf
    ranges[rng.random(ranges.shape) < 0.05] = np.nan
    w = dict(params=p, n_readings=n_readings, max_scans=max_scans, g_first=g_first, pool_offset=offsets, states=states,
             pool_poses=pool_poses, pool_ranges=pool_ranges,
             cand=R.candidates(rows, [c[1] for c in cands], [c[2] for c in cands]), ranges_f32=ranges)
    if seq is not None:
        w["seq"] = seq
    return w


def step(impl, w: dict, edit=None):
    """One round through `impl` (intake, apply, advance): apply runs when the world has "seq"; edit(pool_poses), if
    given, moves poses between apply and advance (AddEdges' weighted mean, the optimiser).  Returns a dict of every
    output."""
    o = impl.intake(w)
    rec, pool = o["rec"], o["pool_poses"]
    if "seq" in w:
        rec, pool = impl.apply(w, rec, w["seq"], pool)
    if edit is not None:
        pool = np.array(pool, copy=True)
        edit(pool)
    adv, states = impl.advance(w, rec, pool)
    return dict(intake=o, rec=rec, pool_poses=pool, adv=adv, states=states)


def next_world(w: dict, out: dict, cands, seq=None) -> dict:
    """The world of the next round: the states and pools `out` left, new candidates (rows 0 .. in order)."""
    n = dict(w)
    n["states"], n["pool_poses"], n["pool_ranges"] = out["states"], out["pool_poses"], out["intake"]["pool_ranges"]
    rows, k = [], 0
    for row, _, _ in cands:
        if row is None:
            row, k = k, k + 1
        rows.append(row)
    n["cand"] = R.candidates(rows, [c[1] for c in cands], [c[2] for c in cands])
    n.pop("seq", None)
    if seq is not None:
        n["seq"] = seq
    return n


def assert_same_step(got: dict, want: dict, what=""):
    R.assert_same_outputs(got["intake"], want["intake"], f"{what} intake")
    for k in ("rec", "pool_poses", "adv", "states"):
        R.assert_same_records(got[k], want[k], f"{what} {k}")


# ------------------------------------------------------------------------------------------------ the gate
HEADING = R.DEFAULT_PARAMS["minimum_travel_heading"]
THR_TRAVEL = 0.2 * 0.2 - R.KT_TOLERANCE
THR_BUFFER = 20.0 * 20.0 - R.KT_TOLERANCE
NAN = math.nan

_dx_at, _dy_at = solve_d2(THR_TRAVEL)
_dx_below, _dy_below = solve_d2(up(THR_TRAVEL, -1))

# name -> (last time, candidate time, candidate odom relative to a last scan at the origin, accepted)
GATE = {
    "time_alone": (0.0, 4000.0, (0.0, 0.0, 0.0), True),
    "heading_alone": (0.0, 1.0, (0.0, 0.0, 0.3), True),
    "distance_alone": (0.0, 1.0, (0.5, 0.0, 0.0), True),
    "nothing": (0.0, 1.0, (0.05, 0.05, 0.05), False),
    "time_exactly_equal": (100.0, 3700.0, (0.0, 0.0, 0.0), True),
    "heading_at_threshold": (0.0, 1.0, (0.0, 0.0, HEADING), True),
    "heading_one_ulp_below": (0.0, 1.0, (0.0, 0.0, up(HEADING, -1)), False),
    "heading_negative_at_threshold": (0.0, 1.0, (0.0, 0.0, -HEADING), True),
    "heading_wraps": (0.0, 1.0, (0.0, 0.0, 2.0 * math.pi - 0.1), False),
    "distance_at_threshold": (0.0, 1.0, (_dx_at, _dy_at, 0.0), True),
    "distance_one_ulp_below": (0.0, 1.0, (_dx_below, _dy_below, 0.0), False),
    "nan_time_still": (0.0, NAN, (0.01, 0.0, 0.0), False),
    "nan_time_moved": (0.0, NAN, (0.5, 0.0, 0.0), True),
    "nan_x": (0.0, 1.0, (NAN, 0.0, 0.0), False),
    "nan_heading": (0.0, 1.0, (0.0, 0.0, NAN), False),
    "inf_heading": (0.0, 1.0, (0.0, 0.0, math.inf), False),
    "nan_x_turned": (0.0, 1.0, (NAN, 0.0, 0.5), True),
}


def case_gate() -> dict:
    """One graph per GATE entry, each with one scan at the origin, then a graph without scans (the first scan)."""
    graphs = [dict(poses=[(0.0, 0.0, 0.0)], last_time=t0) for t0, _, _, _ in GATE.values()] + [dict()]
    cands = [(None, t, odom) for _, t, odom, _ in GATE.values()] + [(None, 5.0, (1.5, -2.0, 0.7))]
    return build_world(graphs, cands, seed=1)


def gate_expected():
    return [acc for _, _, _, acc in GATE.values()] + [True]


# ------------------------------------------------------------------------------------------------ the carry
def case_carry() -> dict:
    """Every scan is accepted by the time clause, so its carried pose reaches the pool.  Graph 0: the last scan's
    corrected pose equals its odometric pose (SetTransform's identity branch); 1: the last odometric pose at the
    origin position with a heading; 2: the general branch; 3: the general branch, across the +-pi cut; 4: a first
    scan whose odometric heading is not normalised; 5: a last pool pose with a NaN."""
    graphs = [dict(poses=[(0.2, 0.1, 0.0), (1.0, 2.0, 0.5)], last_odom=(1.0, 2.0, 0.5)),
              dict(poses=[(1.0, 2.0, 0.5)], last_odom=(0.0, 0.0, 0.3)),
              dict(poses=[(0.0, 0.0, 0.0), (1.1, 2.05, 0.35)], last_odom=(1.0, 2.0, 0.3)),
              dict(poses=[(-3.0, 0.4, 3.1)], last_odom=(-2.5, 0.1, -3.0)),
              dict(),
              dict(poses=[(NAN, 2.0, 0.5)], last_odom=(1.0, 2.0, 0.3))]
    cands = [(None, 4000.0, (1.3, 2.2, 0.6)), (None, 4000.0, (0.4, -0.1, 0.45)), (None, 4000.0, (1.4, 2.1, 0.5)),
             (None, 4000.0, (-2.8, 0.3, 3.05)), (None, 4000.0, (0.5, 0.5, 7.0)), (None, 4000.0, (1.4, 2.1, 0.5))]
    means = [(1.31, 2.19, 0.61), (0.41, -0.1, 0.44), (1.5, 2.2, 0.52), (-3.3, 0.6, -3.12), (1.0, 1.0, 9.0)]
    return build_world(graphs, cands, seed=2, seq=results(means, statuses=[0, 0, R.KT_ERANGE, 0, 0], seed=2))


def moved_sequence():
    """Two rounds on one graph: (first world, the edit after its apply, the second round's candidates).  The optimiser
    moves the scan after the first round's advance, before the second intake reads it."""
    w = build_world([dict(poses=[(0.0, 0.0, 0.0), (0.5, 0.1, 0.1)], last_odom=(0.45, 0.12, 0.08))],
                    [(None, 10.0, (0.9, 0.2, 0.15))], seed=3, seq=results([(1.0, 0.2, 0.2)], seed=3))

    def optimiser(pool):
        pool[2] = (1.08, 0.27, 0.24)

    return w, optimiser, [(None, 20.0, (1.4, 0.3, 0.2))]


# ------------------------------------------------------------------------------------------------ the trim
def _line(n, spacing, far=0, far_at=100.0):
    """n poses along x ending at the origin's neighbourhood; the first `far` of them beyond the buffer distance."""
    poses = [((k - n) * spacing, 0.0, 0.0) for k in range(n)]
    for k in range(far):
        poses[k] = (far_at + k, 0.0, 0.0)
    return poses


def trim_world(poses, params=None, max_scans=16, n_readings=4, run=None, seed=4, at=None):
    """One graph whose last scan sits at its odometric pose (the carry is the identity); the candidate arrives more
    than an hour later with the odometric pose `at` (default: the last scan's), which is then its pool pose exactly,
    and the trim's distances are the front scans' distances to it."""
    g = dict(poses=poses, last_odom=poses[-1])
    if run is not None:
        g["run"] = run
    return build_world([g], [(None, 4000.0, poses[-1] if at is None else at)], params, n_readings, max_scans, seed=seed)


_bx, _by = solve_d2(THR_BUFFER)
_ax, _ay = solve_d2(up(THR_BUFFER, 1))


def trim_cases() -> dict:
    """name -> (world, the window (run_begin, run_length) the advance must leave)."""
    o = (0.0, 0.0, 0.0)
    near3 = [(-0.2, 0.0, 0.0), (-0.1, 0.0, 0.0), o]
    return {
        "nothing_removed": (trim_world(near3), (0, 4)),
        "one_by_size": (trim_world(near3, dict(scan_buffer_size=3)), (1, 3)),
        "one_by_distance": (trim_world([(30.0, 0.0, 0.0), (-0.1, 0.0, 0.0), o]), (1, 3)),
        "d2_at_threshold": (trim_world([(_bx, _by, 0.0), o]), (0, 3)),
        "d2_one_ulp_above": (trim_world([(_ax, _ay, 0.0), o]), (1, 2)),
        "nan_pose_kept": (trim_world([(NAN, 0.0, 0.0), o]), (0, 3)),
        "far_behind_a_near_front": (trim_world([(-0.1, 0.0, 0.0), (50.0, 0.0, 0.0), o]), (0, 4)),
        "all_but_new": (trim_world(near3, at=(100.0, 0.0, 0.0)), (3, 1)),
        "69_of_70": (trim_world(_line(70, 0.01, far=69), max_scans=72), (69, 2)),
        "70_kept": (trim_world(_line(69, 0.01), max_scans=72), (0, 70)),
        "one_of_70_by_size": (trim_world(_line(70, 0.01), max_scans=72), (1, 70)),
        "buffer_size_1": (trim_world(near3, dict(scan_buffer_size=1), run=(2, 1)), (3, 1)),
    }


# ------------------------------------------------------------------------------------------------ refusals
def refused_creates():
    """(params, n_readings, max_scans) kp_create must refuse."""
    d = R.DEFAULT_PARAMS
    return [(dict(d, scan_buffer_size=0), 8, 16), (dict(d, scan_buffer_maximum_scan_distance=0.0005), 8, 16),
            (dict(d, scan_buffer_maximum_scan_distance=NAN), 8, 16), (d, 0, 16), (d, 4097, 16),
            (d, 8, R.KL_MAX_SCANS + 1), (d, 8, 0), (dict(d, minimum_travel_heading=NAN), 8, 16)]


def accepted_creates():
    d = R.DEFAULT_PARAMS
    return [(d, 1, 1), (d, 4096, R.KL_MAX_SCANS), (dict(d, scan_buffer_maximum_scan_distance=0.001), 8, 16),
            (dict(d, scan_buffer_size=1), 8, 16), (dict(R.NODE_PARAMS), 8, 16)]


def case_refusals() -> dict:
    """Graph 0: full (KP_ERANGE); 1: full, but the candidate is rejected by the gate (status KP_OK); 2: its new slot is
    past the pool (KP_EINVAL); 3: absent; 4: a row past n_rows (KP_EINVAL)."""
    four = [(0.1 * k, 0.0, 0.0) for k in range(4)]
    graphs = [dict(poses=four), dict(poses=four), dict(poses=[(0.0, 0.0, 0.0)])] + [dict(poses=four[:2]) for _ in range(2)]
    cands = [(None, 4000.0, (1.0, 0.0, 0.0)), (None, 1.0, (0.3, 0.0, 0.0)), (None, 4000.0, (1.0, 0.0, 0.0)),
             (-1, 4000.0, (1.0, 0.0, 0.0)), (99, 4000.0, (1.0, 0.0, 0.0))]
    w = build_world(graphs, cands, max_scans=4, pool_scans=2 * 5 + 1, seed=5)
    return w


def case_refusals_tail() -> dict:
    """Five graphs of two scans, at slots 5 g and 5 g + 1, over a pool of 16 slots: graphs 0 .. 2 take their scan, graph
    3's last scan (slot 16) and all of graph 4 lie past the pool (KP_EINVAL, nothing read or written there)."""
    four = [(0.1 * k, 0.0, 0.0) for k in range(4)]
    graphs = [dict(poses=four[:2]) for _ in range(5)]
    cands = [(None, 4000.0, (1.0, 0.0, 0.0)) for _ in range(5)]
    return build_world(graphs, cands, max_scans=4, pool_scans=16, seed=6)


# ------------------------------------------------------------------------------------------------ fleets
def fleet_world(n_graphs: int, n_readings: int, seed: int, inverted: int = 0, max_scans: int = 8) -> dict:
    """A fleet with absent, rejected, first and later candidates mixed, windows of every length up to the buffer
    size 4, and matcher results (one in seven KT_ERANGE) for the accepted ones."""
    rng = np.random.default_rng(3000 + seed)
    graphs, cands = [], []
    for g in range(n_graphs):
        n = 0 if (g % 9 == 0 and n_graphs > 1) else int(rng.integers(0, max_scans + 1))
        poses = np.cumsum(rng.normal(0.0, [0.3, 0.3, 0.2], (n, 3)), axis=0)
        spec = dict(poses=poses, last_time=float(rng.uniform(0, 50)))
        if n:
            spec["last_odom"] = poses[-1] + rng.normal(0.0, 0.05, 3)
            length = int(rng.integers(1, min(n, 4) + 1))
            spec["run"] = (n - length, length)
        graphs.append(spec)
        base = spec.get("last_odom", np.zeros(3))
        kind = g % 4 if n_graphs > 1 else 1
        if kind == 0:
            cands.append((-1, 0.0, (0.0, 0.0, 0.0)))
        elif kind == 2:
            cands.append((None, spec["last_time"] + 1.0, tuple(base + [0.01, 0.0, 0.001])))
        else:
            cands.append((None, spec["last_time"] + 2.0, tuple(base + rng.normal(0.0, [0.5, 0.5, 0.4]))))
    w = build_world(graphs, cands, dict(scan_buffer_size=4, scan_buffer_maximum_scan_distance=1.5, inverted=inverted),
                    n_readings, max_scans, seed=seed)
    n = len(cands)
    w["seq"] = results(rng.normal(0.0, 2.0, (n, 3)), statuses=[R.KT_ERANGE if k % 7 == 3 else 0 for k in range(n)], seed=seed)
    return w


def directed_worlds() -> dict:
    """name -> world, for every single-round directed case."""
    d = {"gate": case_gate(), "carry": case_carry(), "refusals": case_refusals(), "refusals_tail": case_refusals_tail()}
    d.update({f"trim_{k}": w for k, (w, _) in trim_cases().items()})
    d["inverted"] = fleet_world(5, 5, 11, inverted=1)
    return d
