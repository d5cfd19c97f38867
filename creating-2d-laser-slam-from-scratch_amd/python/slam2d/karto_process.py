"""Karto's scan-intake stage over the MI355X C-ABI (include/slam2d/karto_process.h).

Reference: what Mapper::Process does before and between the matcher, the candidate search and the linking stage
(lesson6/lib/open_karto/src/Mapper.cpp:2018-2073): the odometry carry, HasMovedEnough (:2087-2120), SetSensorPose
(Karto.h:5289-5300), ScanManager::AddRunningScan (Mapper.h:1365-1386) and the node's readings loop
(lesson6/src/karto_slam.cc:415-440), for a fleet of graphs with one sensor each: `ProcessStage` mirrors the kp_* entry
points one to one.  Results are checked against tests/ref/karto_process_ref.c (parity unpinned against the compiled
library: open_karto needs boost).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib  # noqa: F401  (callers reach the library through the module)
from ._lib import Slam2dError  # noqa: F401
from ._stage import TimedStage, dp as _dp, hp as _hp, library, params_from

KP_OK, KP_EINVAL, KP_EHIP, KP_ENOMEM, KP_ENODEV, KP_ERANGE = 0, -1, -2, -3, -4, -5


class KpParams(C.Structure):
    _fields_ = [("minimum_time_interval", C.c_double), ("minimum_travel_distance", C.c_double),
                ("minimum_travel_heading", C.c_double), ("scan_buffer_maximum_scan_distance", C.c_double),
                ("scan_buffer_size", C.c_int), ("inverted", C.c_int)]


class KpCandidate(C.Structure):
    _fields_ = [("row", C.c_int), ("pad_", C.c_int), ("time", C.c_double), ("odom", C.c_double * 3)]


class KpIntake(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("status", "accepted", "scan", "prev", "job", "seq", "run_begin", "run_length",
                                       "match_status", "pad_")] + [("corrected", C.c_double * 3),
                                                                   ("sensor", C.c_double * 3)]


class KpAdvanced(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("run_begin", "run_length", "n_scans", "accepted")] + [("corrected", C.c_double * 3)]


class KpState(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("n_scans", "run_begin", "run_length", "pad_")] + [
        ("last_time", C.c_double), ("last_odom", C.c_double * 3)]


CANDIDATE_DTYPE = np.dtype([("row", np.int32), ("pad_", np.int32), ("time", np.float64), ("odom", np.float64, 3)])
INTAKE_DTYPE = np.dtype([(k, np.int32) for k, _ in KpIntake._fields_[:10]] + [("corrected", np.float64, 3),
                                                                             ("sensor", np.float64, 3)])
ADVANCED_DTYPE = np.dtype([(k, np.int32) for k, _ in KpAdvanced._fields_[:4]] + [("corrected", np.float64, 3)])
STATE_DTYPE = np.dtype([(k, np.int32) for k, _ in KpState._fields_[:4]] + [("last_time", np.float64),
                                                                          ("last_odom", np.float64, 3)])
assert CANDIDATE_DTYPE.itemsize == C.sizeof(KpCandidate) and INTAKE_DTYPE.itemsize == C.sizeof(KpIntake)
assert ADVANCED_DTYPE.itemsize == C.sizeof(KpAdvanced) and STATE_DTYPE.itemsize == C.sizeof(KpState)


def _declare(L):
    if getattr(L, "_kp_declared", False):
        return
    vp, i, P = C.c_void_p, C.c_int, C.POINTER
    L.kp_last_error.restype = C.c_char_p
    L.kp_version.restype = C.c_char_p
    L.kp_default_params.restype = None
    L.kp_default_params.argtypes = [P(KpParams)]
    L.kp_node_params.restype = None
    L.kp_node_params.argtypes = [P(KpParams)]
    L.kp_create.argtypes = [P(vp), P(KpParams), i, i, i, vp]
    L.kp_destroy.argtypes = [vp]
    L.kp_intake_device.argtypes = [vp, i, i, vp, vp, i, vp, vp, i, vp, vp, vp, i, vp, vp, vp, vp, vp, vp]
    L.kp_apply_match_device.argtypes = [vp, vp, i, vp, i, vp]
    L.kp_commit_vertices.argtypes = [vp, vp, vp, P(i)]
    L.kp_bind_near_device.argtypes = [vp, vp, vp, vp, i, vp]
    L.kp_advance_device.argtypes = [vp, vp, i, vp]
    L.kp_get_intake.argtypes = [vp, i, i, vp, vp]
    L.kp_result_device.argtypes = [vp, P(vp), P(vp), P(vp), P(vp)]
    L.kp_get_state.argtypes = [vp, i, vp]
    L.kp_set_state.argtypes = [vp, i, vp]
    L.kp_clear_graph.argtypes = [vp, i]
    L.kp_set_timing.argtypes = [vp, i]
    L.kp_num_kernels.restype = i
    L.kp_kernel_name.restype = C.c_char_p
    L.kp_kernel_name.argtypes = [i]
    L.kp_get_kernel_times.argtypes = [vp, vp, vp, i]
    L._kp_declared = True


def default_params(**kw) -> KpParams:
    """kp_default_params: the Mapper defaults (3600, 0.2, DegreesToRadians(10), 20, 70, not inverted); keywords
    override."""
    return params_from(library(_declare), KpParams, "kp_default_params", **kw)


def node_params(**kw) -> KpParams:
    """kp_node_params: mapper_params.yaml (3600, 0.2, 0.174, 100, 110, not inverted); keywords override."""
    return params_from(library(_declare), KpParams, "kp_node_params", **kw)


def candidates(rows, times, odoms) -> np.ndarray:
    """A kp_candidate array from rows [n] (negative: absent), times [n] and odometric poses [n, 3]."""
    rows = np.asarray(rows, np.int32).reshape(-1)
    c = np.zeros(len(rows), CANDIDATE_DTYPE)
    c["row"] = rows
    c["time"] = np.asarray(times, np.float64).reshape(-1)
    c["odom"] = np.asarray(odoms, np.float64).reshape(-1, 3)
    return c


class ProcessStage(TimedStage):
    """The intake state of `n_graphs` graphs of up to `max_scans` scans of `n_readings` readings; graph g's scan i is
    pool slot pool_offset[g] + i (None: g * max_scans).  Device pointers are ints."""

    _PREFIX = "kp"

    def __init__(self, params: KpParams | None, n_graphs: int, n_readings: int, max_scans: int, pool_offset=None):
        self.L = library(_declare)
        self.params = params if params is not None else default_params()
        self.n_graphs, self.n_readings, self.max_scans = int(n_graphs), int(n_readings), int(max_scans)
        off = None
        if pool_offset is not None:
            off = np.ascontiguousarray(pool_offset, np.int32).reshape(-1)
            if len(off) != self.n_graphs:
                raise ValueError("pool_offset needs one entry per graph")
        self.h = C.c_void_p()
        self._check(self.L.kp_create(C.byref(self.h), C.byref(self.params), self.n_graphs, self.n_readings,
                                     self.max_scans, _hp(off) if off is not None else None), "kp_create")

    # ------------------------------------------------------------------------------------------------ the stages
    def intake_device(self, g_first: int, count: int, d_candidates: int, d_ranges_f32: int, n_rows: int,
                      d_pool_ranges: int, d_pool_poses: int, pool_scans: int, d_query: int, d_base_begin: int,
                      d_base_index: int, base_capacity: int, d_n_seq: int, d_jobs: int, d_queries: int, d_n_jobs: int,
                      d_closest_items: int, hip_stream: int = 0):
        self._check(self.L.kp_intake_device(
            self.h, int(g_first), int(count), _dp(d_candidates), _dp(d_ranges_f32), int(n_rows), _dp(d_pool_ranges),
            _dp(d_pool_poses), int(pool_scans), _dp(d_query), _dp(d_base_begin), _dp(d_base_index), int(base_capacity),
            _dp(d_n_seq), _dp(d_jobs), _dp(d_queries), _dp(d_n_jobs), _dp(d_closest_items), _dp(hip_stream)),
            "kp_intake_device")

    def apply_match_device(self, d_seq: int, n_seq: int, d_pool_poses: int, pool_scans: int, hip_stream: int = 0):
        self._check(self.L.kp_apply_match_device(self.h, _dp(d_seq), int(n_seq), _dp(d_pool_poses), int(pool_scans),
                                                 _dp(hip_stream)), "kp_apply_match_device")

    def commit_vertices(self, loop_fleet, spa_fleet) -> int:
        """kp_commit_vertices into a LoopSearchFleet and (or None) a SpaFleet; the number of vertices added."""
        n = C.c_int(0)
        spa_h = spa_fleet.h if spa_fleet is not None else None
        self._check(self.L.kp_commit_vertices(self.h, loop_fleet.h, spa_h, C.byref(n)), "kp_commit_vertices")
        return n.value

    def bind_near_device(self, d_jobs: int, d_source: int, d_n_matches: int, max_matches: int, hip_stream: int = 0):
        self._check(self.L.kp_bind_near_device(self.h, _dp(d_jobs), _dp(d_source), _dp(d_n_matches), int(max_matches),
                                               _dp(hip_stream)), "kp_bind_near_device")

    def advance_device(self, d_pool_poses: int, pool_scans: int, hip_stream: int = 0):
        self._check(self.L.kp_advance_device(self.h, _dp(d_pool_poses), int(pool_scans), _dp(hip_stream)),
                    "kp_advance_device")

    # ------------------------------------------------------------------------------------------------ the results
    def get_intake(self, first: int, count: int):
        """(records [count] of INTAKE_DTYPE, advance records [count] of ADVANCED_DTYPE) of the last calls."""
        rec, adv = np.zeros(count, INTAKE_DTYPE), np.zeros(count, ADVANCED_DTYPE)
        self._check(self.L.kp_get_intake(self.h, int(first), int(count), _hp(rec), _hp(adv)), "kp_get_intake")
        return rec, adv

    def result_device(self) -> dict:
        """Device addresses of the intake records, the advance records, the graph states and the two counts."""
        a, b, s, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.L.kp_result_device(self.h, C.byref(a), C.byref(b), C.byref(s), C.byref(n)), "kp_result_device")
        return {"intake": int(a.value or 0), "advanced": int(b.value or 0), "state": int(s.value or 0),
                "counts": int(n.value or 0)}

    def get_state(self, g: int) -> np.ndarray:
        s = np.zeros(1, STATE_DTYPE)
        self._check(self.L.kp_get_state(self.h, int(g), _hp(s)), "kp_get_state")
        return s[0]

    def set_state(self, g: int, n_scans: int, run_begin: int, run_length: int, last_time: float, last_odom):
        s = np.zeros(1, STATE_DTYPE)
        s[0] = (n_scans, run_begin, run_length, 0, last_time, np.asarray(last_odom, np.float64).reshape(3))
        self._check(self.L.kp_set_state(self.h, int(g), _hp(s)), "kp_set_state")

    def clear_graph(self, g: int):
        self._check(self.L.kp_clear_graph(self.h, int(g)), "kp_clear_graph")
