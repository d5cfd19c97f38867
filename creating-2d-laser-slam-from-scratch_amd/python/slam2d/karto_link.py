"""Karto's graph-linking stage over the MI355X C-ABI (include/slam2d/karto_link.h).

Reference: MapperGraph::AddEdges, TryCloseLoop's accept / reject tests, LinkScans / LinkInfo, SpaSolver::AddConstraint's
precision matrix and ComputeWeightedMean (lesson6/lib/open_karto/src/Mapper.cpp:902-1167, :1288-1330; Mapper.h:138-152;
lesson6/src/spa_solver/spa_solver.cc:70-91) for a fleet of graphs, from the device-resident results of the matcher
(karto.py) and the candidate search (karto_loop.py): `LinkStage` mirrors the ke_* entry points one to one.  Results are
checked against tests/ref/karto_link_ref.c (parity unpinned against the compiled library: open_karto needs boost).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib  # noqa: F401  (callers reach the library through the module)
from ._lib import Slam2dError  # noqa: F401
from ._stage import TimedStage, dp as _dp, hp as _hp, library, params_from
from .karto import RESULT_DTYPE as KT_RESULT_DTYPE  # noqa: F401

KE_OK, KE_EINVAL, KE_EHIP, KE_ENOMEM, KE_ENODEV, KE_ERANGE, KE_SINGULAR = 0, -1, -2, -3, -4, -5, -6
KE_MAX_LINKS = 64
KE_PREV, KE_RUNNING, KE_NEAR, KE_LOOP = 0, 1, 2, 3
KE_WRITE_POSE = 1
KE_LOOP_OVERFLOW, KE_LOOP_EINVAL = 1, 2


class KeParams(C.Structure):
    _fields_ = [("link_match_minimum_response_fine", C.c_double), ("loop_match_minimum_response_coarse", C.c_double),
                ("loop_match_maximum_variance_coarse", C.c_double), ("loop_match_minimum_response_fine", C.c_double)]


class KeJob(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("graph", "scan", "pool_offset", "prev", "seq_result", "running", "near_first",
                                       "near_count")]


class KeLink(C.Structure):
    _fields_ = [("from_", C.c_int), ("to", C.c_int), ("kind", C.c_int), ("status", C.c_int), ("diff", C.c_double * 3),
                ("precision", C.c_double * 9)]


class KeJobOut(C.Structure):
    _fields_ = [("n_links", C.c_int), ("n_means", C.c_int), ("status", C.c_int), ("graph", C.c_int),
                ("pose", C.c_double * 3)]


class KeClosure(C.Structure):
    _fields_ = [("chain", C.c_int), ("resume", C.c_int), ("fine", C.c_int), ("pad_", C.c_int), ("pose", C.c_double * 3),
                ("covariance", C.c_double * 9)]


JOB_DTYPE = np.dtype([(k, np.int32) for k, _ in KeJob._fields_])
LINK_DTYPE = np.dtype([("from", np.int32), ("to", np.int32), ("kind", np.int32), ("status", np.int32),
                       ("diff", np.float64, 3), ("precision", np.float64, 9)])
JOB_OUT_DTYPE = np.dtype([("n_links", np.int32), ("n_means", np.int32), ("status", np.int32), ("graph", np.int32),
                          ("pose", np.float64, 3)])
CLOSURE_DTYPE = np.dtype([("chain", np.int32), ("resume", np.int32), ("fine", np.int32), ("pad_", np.int32),
                          ("pose", np.float64, 3), ("covariance", np.float64, 9)])
assert JOB_DTYPE.itemsize == C.sizeof(KeJob) and LINK_DTYPE.itemsize == C.sizeof(KeLink)
assert JOB_OUT_DTYPE.itemsize == C.sizeof(KeJobOut) and CLOSURE_DTYPE.itemsize == C.sizeof(KeClosure)


def _declare(L):
    if getattr(L, "_ke_declared", False):
        return
    vp, i, P = C.c_void_p, C.c_int, C.POINTER
    L.ke_last_error.restype = C.c_char_p
    L.ke_version.restype = C.c_char_p
    L.ke_default_params.restype = None
    L.ke_default_params.argtypes = [P(KeParams)]
    L.ke_node_params.restype = None
    L.ke_node_params.argtypes = [P(KeParams)]
    L.ke_create.argtypes = [P(vp), P(KeParams), i, i, i, i]
    L.ke_destroy.argtypes = [vp]
    L.ke_add_edges_device.argtypes = [vp, i, vp, vp, i, vp, i, vp, i, vp, vp, i, vp, i, i, i, vp]
    L.ke_loop_coarse_device.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ke_get_loop_info.argtypes = [vp, P(i), P(i)]
    L.ke_loop_fine_device.argtypes = [vp, i, i, vp, vp, vp, i, vp, vp, vp, i, vp, vp, i, i, vp]
    L.ke_close_device.argtypes = [vp, i, vp, vp, vp, vp, i, vp]
    L.ke_get_links.argtypes = [vp, i, i, vp, vp]
    L.ke_result_device.argtypes = [vp, P(vp), P(vp), P(i)]
    L.ke_commit.argtypes = [vp, vp, vp, i, i, P(i)]
    L.ke_set_timing.argtypes = [vp, i]
    L.ke_num_kernels.restype = i
    L.ke_kernel_name.restype = C.c_char_p
    L.ke_kernel_name.argtypes = [i]
    L.ke_get_kernel_times.argtypes = [vp, vp, vp, i]
    L._ke_declared = True


def default_params(**kw) -> KeParams:
    """ke_default_params: the Mapper defaults (0.8, 0.8, 0.4 * 0.4, 0.8); keywords override."""
    return params_from(library(_declare), KeParams, "ke_default_params", **kw)


def node_params(**kw) -> KeParams:
    """ke_node_params: mapper_params.yaml (0.1, 0.35, 3.0 * 3.0, 0.45); keywords override."""
    return params_from(library(_declare), KeParams, "ke_node_params", **kw)


def jobs(rows) -> np.ndarray:
    """rows of (graph, scan, pool_offset, prev, seq_result, running, near_first, near_count) -> a ke_job array."""
    a = np.ascontiguousarray(rows, np.int32).reshape(-1, 8)
    return np.ascontiguousarray(a).view(JOB_DTYPE).reshape(-1)


class LinkStage(TimedStage):
    """Link rows for `max_jobs` jobs of at most `max_links` records, scans of `n_readings` readings and loop batches
    of at most `max_matches` coarse matches.  Device pointers are ints."""

    _PREFIX = "ke"

    def __init__(self, params: KeParams | None, n_readings: int, max_jobs: int, max_links: int = KE_MAX_LINKS,
                 max_matches: int = 1):
        self.L = library(_declare)
        self.params = params if params is not None else default_params()
        self.n_readings, self.max_jobs = int(n_readings), int(max_jobs)
        self.max_links, self.max_matches = int(max_links), int(max_matches)
        self.h = C.c_void_p()
        self._check(self.L.ke_create(C.byref(self.h), C.byref(self.params), self.n_readings, self.max_jobs,
                                     self.max_links, self.max_matches), "ke_create")

    # ------------------------------------------------------------------------------------------------ the stages
    def add_edges_device(self, count: int, d_jobs: int, d_pool_poses: int, pool_scans: int, d_seq: int, n_seq: int,
                         d_running: int, n_running: int, d_near: int, d_near_source: int, n_near: int,
                         d_near_chains: int, chain_stride: int, n_slots: int, flags: int = 0, hip_stream: int = 0):
        self._check(self.L.ke_add_edges_device(self.h, int(count), _dp(d_jobs), _dp(d_pool_poses), int(pool_scans),
                                               _dp(d_seq), int(n_seq), _dp(d_running), int(n_running), _dp(d_near),
                                               _dp(d_near_source), int(n_near), _dp(d_near_chains), int(chain_stride),
                                               int(n_slots), int(flags), _dp(hip_stream)), "ke_add_edges_device")

    def loop_coarse_device(self, max_matches: int, d_n_matches: int, d_coarse: int, d_query: int, d_base_begin: int,
                           d_base_index: int, d_pool_ranges: int, pool_scans: int, tmp_first: int, capacity: int,
                           base_capacity: int, d_fine_query: int, d_fine_base_begin: int, d_fine_base_index: int,
                           d_fine_of: int, d_n_fine: int, d_tmp_ranges: int, d_tmp_poses: int, hip_stream: int = 0):
        self._check(self.L.ke_loop_coarse_device(
            self.h, int(max_matches), _dp(d_n_matches), _dp(d_coarse), _dp(d_query), _dp(d_base_begin),
            _dp(d_base_index), _dp(d_pool_ranges), int(pool_scans), int(tmp_first), int(capacity), int(base_capacity),
            _dp(d_fine_query), _dp(d_fine_base_begin), _dp(d_fine_base_index), _dp(d_fine_of), _dp(d_n_fine),
            _dp(d_tmp_ranges), _dp(d_tmp_poses), _dp(hip_stream)), "ke_loop_coarse_device")

    def loop_info(self):
        """(accepted matches before the capacity cut, status bits) of the last coarse call."""
        total, status = C.c_int(0), C.c_int(0)
        self._check(self.L.ke_get_loop_info(self.h, C.byref(total), C.byref(status)), "ke_get_loop_info")
        return total.value, status.value

    def loop_fine_device(self, count: int, capacity: int, d_n_fine: int, d_fine: int, d_fine_of: int, max_matches: int,
                         d_source: int, d_query: int, d_loop_chains: int, chain_stride: int, d_closures: int,
                         d_pool_poses: int = 0, pool_scans: int = 0, flags: int = 0, hip_stream: int = 0):
        self._check(self.L.ke_loop_fine_device(
            self.h, int(count), int(capacity), _dp(d_n_fine), _dp(d_fine), _dp(d_fine_of), int(max_matches),
            _dp(d_source), _dp(d_query), _dp(d_loop_chains), int(chain_stride), _dp(d_closures), _dp(d_pool_poses),
            int(pool_scans), int(flags), _dp(hip_stream)), "ke_loop_fine_device")

    def close_device(self, count: int, d_jobs: int, d_closures: int, d_closest: int, d_pool_poses: int,
                     pool_scans: int, hip_stream: int = 0):
        self._check(self.L.ke_close_device(self.h, int(count), _dp(d_jobs), _dp(d_closures), _dp(d_closest),
                                           _dp(d_pool_poses), int(pool_scans), _dp(hip_stream)), "ke_close_device")

    # ------------------------------------------------------------------------------------------------ the results
    def get_links(self, first_job: int, count: int):
        """(links [count, max_links] of LINK_DTYPE, jobs [count] of JOB_OUT_DTYPE) of the last stage-1 / stage-3 call;
        only the first n_links records of a row are defined."""
        links = np.zeros((count, self.max_links), LINK_DTYPE)
        out = np.zeros(count, JOB_OUT_DTYPE)
        self._check(self.L.ke_get_links(self.h, int(first_job), int(count), _hp(links), _hp(out)), "ke_get_links")
        return links, out

    def result_device(self) -> dict:
        """Device addresses of the link rows and the job outputs."""
        a, b, k = C.c_void_p(), C.c_void_p(), C.c_int(0)
        self._check(self.L.ke_result_device(self.h, C.byref(a), C.byref(b), C.byref(k)), "ke_result_device")
        return {"links": int(a.value or 0), "jobs_out": int(b.value or 0), "max_links": k.value}

    def commit(self, loop_fleet, spa_fleet, first_job: int, count: int) -> int:
        """ke_commit into a LoopSearchFleet and (or None) a SpaFleet; the number of new edges."""
        n = C.c_int(0)
        spa_h = spa_fleet.h if spa_fleet is not None else None
        self._check(self.L.ke_commit(self.h, loop_fleet.h, spa_h, int(first_job), int(count), C.byref(n)), "ke_commit")
        return n.value
