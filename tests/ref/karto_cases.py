"""Inputs of the Karto matcher's path tests, shared by tests/test_karto_paths_gpu.py (the kt_* kernels against
oracle/karto_oracle.c) and test_path_case_preconditions in tests/test_karto_cpu.py (the oracle alone): every case
is built once here, so the precondition that makes a case reach its kernel path is asserted on the very inputs the
GPU test runs.  Plain module (no fixtures); everything is cached, nothing is mutated after it is built.

Laser and parameters are the oracle's ctypes structures (oracle.KtLaser / oracle.KtParams); the product's have the
same fields in the same order.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

import oracle as O
from slam2d import synth

D = math.pi / 180.0
SPAN = 270.0 * D  # every laser here sweeps the same 270 degrees as synth's 1081 beams

# smear_deviation -> smear kernel size at resolution 0.01 (checked by test_path_case_preconditions); with the
# sequential default (13) and the loop matcher's 3 (0.03 at 0.05 m) they reach every smear branch:
#   kt_group:            ks <= 15 per-lane cell tables | ks > 15 lane-strided generic smear
#   kt_addscans_kernel:  ks <= 13 dword render | ks = 15 kt_render_items<4> | ks > 15 bounds-tested (17: half 8 fits
#                        the 16-cell LDS margin, 35 / 41: half 17 / 20 exceeds it)
SMEAR = {3: 0.005, 13: 0.03, 15: 0.035, 17: 0.04, 35: 0.085, 41: 0.099}
SMEAR_KEYS = [3, 13, 15, 17, 35, 41, "loop"]  # "loop": the loop matcher's 0.05 m grid, ksize 3
SHORT_N = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257]
KT_AS_ITEMS = 15360  # kt_addscans_kernel's item store: more footprint items per match need a second pass


def laser(n=synth.N_BEAMS, thr=12.0, min_range=0.1, ang_res=None) -> O.KtLaser:
    if ang_res is None:
        ang_res = float(synth.ANGLE_INC) if n == synth.N_BEAMS else SPAN / max(n - 1, 1)
    return O.KtLaser(float(synth.ANGLE_MIN), float(ang_res), float(min_range), float(thr), int(n), 0)


def params(loop=False, **over) -> O.KtParams:
    """Mapper::InitializeParameters (Mapper.cpp:1569-1660), then the overrides."""
    p = O.KtParams(8.0 if loop else 0.3, 0.05 if loop else 0.01, 0.03, 0.3 ** 2, (20 * D) ** 2, 0.2 * D, 20 * D, 2 * D,
                   0.9, 0.5, 0, 0)
    for k, v in over.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def smear_params(key) -> O.KtParams:
    if key == "loop":
        return params(loop=True, search_size=2.0)  # 21 x 21 coarse positions
    return params(smear_deviation=SMEAR[key])


def beam_angles(lz: O.KtLaser) -> np.ndarray:
    return lz.minimum_angle + np.arange(lz.n_readings, dtype=np.float64) * lz.angular_resolution


@dataclass(frozen=True)
class Case:
    """One MatchScan call: a query and its (possibly empty) list of base scans."""
    name: str
    laser: O.KtLaser
    params: O.KtParams
    q_ranges: np.ndarray  # [n]
    q_pose: np.ndarray    # [3]
    b_ranges: np.ndarray  # [B, n]
    b_poses: np.ndarray   # [B, 3]
    penalize: bool = True
    refine: bool = True

    def match(self, **over):
        kw = dict(penalize=self.penalize, refine=self.refine)
        kw.update(over)
        return O.karto_match(self.laser, self.params, self.q_ranges, self.q_pose, self.b_ranges, self.b_poses,
                             kw["penalize"], kw["refine"])

    def count_valid(self) -> np.ndarray:
        return O.karto_count_valid(self.laser, self.params, self.q_pose, self.b_ranges, self.b_poses)

    def with_params(self, name, **over):
        p = O.KtParams.from_buffer_copy(self.params)
        for k, v in over.items():
            assert hasattr(p, k), k
            setattr(p, k, v)
        return Case(name, self.laser, p, self.q_ranges, self.q_pose, self.b_ranges, self.b_poses, self.penalize,
                    self.refine)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------ batches
@dataclass(frozen=True)
class Batch:
    """`M` matches over pooled scans, as kt_match_batch_device takes them: pool slots [0, S) hold the true-pose
    scans (the bases), [S, S + M) the queries at their odometry poses; match i has counts[i] base scans."""
    pool_ranges: np.ndarray  # [S + M, n]
    pool_poses: np.ndarray   # [S + M, 3]
    query: np.ndarray        # [M] int32
    begin: np.ndarray        # [M + 1] int32
    index: np.ndarray        # [sum counts] int32
    max_base: int

    @property
    def count(self):
        return self.query.shape[0]

    def case(self, i, lz, p, **kw) -> Case:
        idx = self.index[self.begin[i]:self.begin[i + 1]]
        return Case(f"match{i}", lz, p, self.pool_ranges[self.query[i]], self.pool_poses[self.query[i]],
                    self.pool_ranges[idx], self.pool_poses[idx], **kw)


@functools.lru_cache(maxsize=None)
def sequential_batch(M, B, seed=9) -> Batch:
    """synth.karto_sequential(M, B): match i is scan B + i against the B - (i mod 3) scans before it (ragged)."""
    R, T, Q = synth.karto_sequential(M, B, seed=seed)
    S = R.shape[0]
    counts = [B - (i % 3) for i in range(M)]
    beg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    idx = np.concatenate([np.arange(B + i - c, B + i) for i, c in enumerate(counts)]).astype(np.int32)
    return Batch(*_freeze(np.concatenate([R, R[B:]]), np.concatenate([T, Q[B:]]), np.arange(S, S + M, dtype=np.int32),
                          beg, idx), B)


@functools.lru_cache(maxsize=None)
def loop_batch(M, K, seed=17) -> Batch:
    """synth.karto_loop(M, K): query i against its own chain of K first-lap scans."""
    QR, qp, _, CR, CP = synth.karto_loop(M, K, seed=seed, perturb=(0.2, 0.2, 0.03))
    n = QR.shape[1]
    return Batch(*_freeze(np.concatenate([QR, CR.reshape(-1, n)]), np.concatenate([qp, CP.reshape(-1, 3)]),
                          np.arange(M, dtype=np.int32), (np.arange(M + 1) * K).astype(np.int32),
                          np.arange(M, M + M * K, dtype=np.int32)), K)


def smear_batch(M) -> Batch:
    """The batch of the smear-size grid tests: 6 / 5 / 4 base scans per match (one pass of kt_addscans_kernel)."""
    return sequential_batch(M, 6)


def many_base_batch() -> Batch:
    """32 / 31 / 30 base scans per match: more than KT_AS_ITEMS valid points, so kt_addscans_kernel takes a second
    pass and re-reads the tiles the first one wrote (its `was` branch)."""
    return sequential_batch(128, 32)


# ------------------------------------------------------------------------------------------ single cases
@functools.lru_cache(maxsize=None)
def dense() -> Case:
    """4096 beams over the same 270 degrees, range_threshold 20, no noise: five base scans and a copy of base scan
    4 at its true pose.  More than 2045 valid query points at a response close to 1 (the 16-bit flush of
    kt_coarse_kernel), n_readings >= 2731 (kt_prepare_kernel above 64 KB of LDS), more than 3072 points (the fourth
    register round of kt_fine_kernel)."""
    lz = laser(4096, thr=20.0)
    poses = synth.trajectory(12, 0.3)[::2]
    R = synth.cast_ranges(poses, synth.world_segments(), 4096, angles=beam_angles(lz))
    return Case("dense", lz, params(), *_freeze(R[4].copy(), poses[4].copy(), R[:5].copy(), poses[:5].copy()))


@functools.lru_cache(maxsize=None)
def expansion() -> dict:
    """A 62-beam wall patch 6 m away as the only in-range readings, query = the same readings at the true pose with
    the heading off by 0 / 50 / 70 / 90 degrees, response expansion on: the coarse window of +-20 degrees sees
    nothing for the rotated ones, and MatchScan widens it by 20 degrees per pass until an edge of the patch comes
    into reach (at +-40, +-60 and +-80 degrees: pass 1, 2 and 3)."""
    R, T, _ = synth.karto_sequential(1, 2, seed=3, noise=0.0)
    r = np.full(R.shape[1], 25.0)  # 25.0, not inf: the reference indexes the raw readings with the point number
    r[813:875] = R[0, 813:875]
    lz, p = laser(), params(use_response_expansion=1)
    out = {}
    for deg in (0, 50, 70, 90):
        q = T[0] + np.array([0.0, 0.0, deg * D])
        out[deg] = Case(f"expansion{deg}", lz, p, *_freeze(r.copy(), q, r[None].copy(), T[:1].copy()))
    return out


HEADING_SHIFTS = [0.0, 6 * math.pi, -8 * math.pi]


@functools.lru_cache(maxsize=None)
def headings() -> list:
    """Four sequential matches whose headings run 3.04 .. pi .. -3.11 (scan 7 is at pi exactly), each also with the
    query heading shifted by +6 pi and -8 pi (unnormalised)."""
    step, dt = 2, 0.08 / 6.7
    R, T, Q = synth.karto_sequential(4, 6, seed=5, phase=math.pi / 2 - 7 * step * dt)
    lz, p = laser(), params()
    out = []
    for i in range(6, 10):
        for s in HEADING_SHIFTS:
            q = Q[i] + np.array([0.0, 0.0, s])
            out.append(Case(f"heading{i}{s / math.pi:+.0f}pi", lz, p, *_freeze(R[i].copy(), q, R[i - 6:i].copy(), T[i - 6:i].copy())))
    return out


@functools.lru_cache(maxsize=None)
def short(n) -> list:
    """Two matches of `n` beams over 270 degrees against three base scans: the points are metres apart, so a chunk
    of 16 (or a quarter of 4) does not fit kt_build_kernel's 96 x 96-cell LDS tile."""
    lz = laser(n)
    poses = synth.trajectory(10, 0.3)[::2]
    R = synth.cast_ranges(poses, synth.world_segments(), n, angles=beam_angles(lz))
    out = []
    for i in (3, 4):
        q = poses[i] + np.array([0.02, -0.03, 0.01])
        out.append(Case(f"short{n}_{i}", lz, params(), *_freeze(R[i].copy(), q, R[i - 3:i].copy(), poses[i - 3:i].copy())))
    return out


@functools.lru_cache(maxsize=None)
def degenerate() -> dict:
    R, T, Q = synth.karto_sequential(2, 3, seed=13)
    lz, p = laser(), params()
    none = np.full(R.shape[1], 25.0)  # every reading out of range
    out = {}
    # a query with no valid point against a non-empty grid: every response is 0 / 0 -> 0
    out["query_out_of_range"] = Case("query_out_of_range", lz, p, none, Q[3], R[:3], T[:3])
    # a base scan with no in-range reading between two ordinary ones
    out["empty_base"] = Case("empty_base", lz, p, R[3], Q[3], np.stack([R[0], none, R[2]]), T[:3])
    # a base scan seen from behind: only a wall patch is in range, and the query stands beyond that wall, so every
    # point of it is on the wrong side of the viewpoint (FindValidPoints, Mapper.cpp:795-799)
    patch = none.copy()
    patch[813:875] = R[0, 813:875]
    ang = T[0, 2] + beam_angles(lz)[844]
    behind = T[0] + np.array([math.cos(ang), math.sin(ang), 0.0]) * (R[0, 844] + 2.0)
    out["base_from_behind"] = Case("base_from_behind", lz, p, R[3], behind, np.stack([patch, R[1]]), T[:2])
    # a base scan 15 m from the query: its points are partly outside the ROI (12.15 m around the query)
    far = synth.trajectory(1, math.pi + 0.3)
    FR = synth.cast_ranges(far, synth.world_segments())
    out["base_partly_outside"] = Case("base_partly_outside", lz, p, R[3], Q[3], np.stack([R[2], FR[0]]),
                                      np.stack([T[2], far[0]]))
    # minimum_range 3.0 drops the near readings of every scan; the loop trajectory stays 3 m clear of everything,
    # so these scans are taken 1.5 m from the central box
    near = np.array([[0.1 * i, 2.5, 0.2 * i] for i in range(4)])
    NR = synth.cast_ranges(near, synth.world_segments())
    out["minimum_range"] = Case("minimum_range", laser(min_range=3.0), p, NR[3], near[3] + np.array([0.02, 0.01, 0.01]),
                                NR[:3], near[:3])
    # no base scans on the loop matcher's windows: every pose ties at 0 (441 x 21 and 6561 x 21 ties: more than
    # one round of kt_select_kernel's tie compaction)
    out["all_tie_21"] = Case("all_tie_21", lz, params(loop=True, search_size=2.0), R[3], Q[3], R[:0], T[:0], False, False)
    out["all_tie_81"] = Case("all_tie_81", lz, params(loop=True), R[3], Q[3], R[:0], T[:0], False, True)
    for c in out.values():
        _freeze(c.q_ranges, c.q_pose, c.b_ranges, c.b_poses)
    return out


# ------------------------------------------------------------------------------------------ plain restatement
def find_valid_points(lz: O.KtLaser, ranges, pose, viewpoint):
    """FindValidPoints (Mapper.cpp:755-811) on the point readings of LocalizedRangeScan::Update, restated plainly:
    returns (points [npts, 2], valid [npts])."""
    r = np.asarray(ranges, np.float64)
    keep = (r >= lz.minimum_range) & (r <= lz.range_threshold)
    a = pose[2] + beam_angles(lz)[keep]
    pts = np.stack([pose[0] + r[keep] * np.cos(a), pose[1] + r[keep] * np.sin(a)], axis=1)
    valid = np.zeros(len(pts), bool)
    trailing, first = 0, None
    for k, (cx, cy) in enumerate(pts):
        if first is None:
            first = (cx, cy)
        fx, fy = first
        if (fx - cx) ** 2 + (fy - cy) ** 2 > 0.1 * 0.1:
            ss = cx * (viewpoint[1] - fy) + cy * (fx - viewpoint[0]) + (fy * viewpoint[0] - fx * viewpoint[1])
            first = (cx, cy)
            if ss < 0.0:
                trailing = k
            else:
                valid[trailing:k] = True
                trailing = k
    return pts, valid


def roi_cells(c: Case, pts):
    """AddScan's cells of `pts` in the grid centred on the case's query pose, and which of them lie in the ROI."""
    g = O.karto_grid_info(c.params, c.laser)
    scale = 1.0 / c.params.resolution
    org = np.asarray(c.q_pose[:2]) - 0.5 * (g["grid_size"] - 1) * (1.0 / scale)
    cells = np.floor((pts - org) * scale + 0.5).astype(np.int64)
    inside = ((cells >= 0) & (cells < g["grid_size"])).all(axis=1)
    return cells + g["border"], inside


def footprint_items(c: Case, b) -> int:
    """Items base scan `b` puts into kt_addscans_kernel's store: the 64 x 64 tiles its footprints overlap."""
    pts, valid = find_valid_points(c.laser, c.b_ranges[b], c.b_poses[b], c.q_pose[:2])
    cells, inside = roi_cells(c, pts)
    cells = cells[valid & inside]
    h = O.karto_grid_info(c.params, c.laser)["half"]
    span = ((cells + h) >> 6) - ((cells - h) >> 6) + 1
    return int((span[:, 0] * span[:, 1]).sum())
