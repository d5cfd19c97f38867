"""Karto's graph-edit stage over the MI355X C-ABI (include/slam2d/karto_edit.h).

Reference: the AddVertex / AddNode calls of Mapper::Process (lesson6/lib/open_karto/src/Mapper.cpp:2053) and the
AddEdge / AddConstraint calls of LinkScans (:1104-1121), applied to the device-resident graphs of a `LoopSearchFleet`
and a `SpaFleet` from the device-resident records of a `ProcessStage` and a `LinkStage`, with no host step in between:
`GraphEdits` mirrors the kd_* entry points one to one.  Results are checked against the host commits
(kp_commit_vertices, ke_commit) bit for bit.
"""
from __future__ import annotations

import ctypes as C

from . import _lib  # noqa: F401  (callers reach the library through the module)
from ._lib import Slam2dError  # noqa: F401
from ._stage import TimedStage, dp as _dp, library
from . import karto_loop as _kl
from . import spa as _spa

KD_OK, KD_EINVAL, KD_EHIP, KD_ENOMEM, KD_ENODEV, KD_ERANGE = 0, -1, -2, -3, -4, -5


def _declare(L):
    if getattr(L, "_kd_declared", False):
        return
    vp, i, P = C.c_void_p, C.c_int, C.POINTER
    _kl._declare(L)
    _spa._declare(L)
    L.kd_last_error.restype = C.c_char_p
    L.kd_version.restype = C.c_char_p
    L.kd_create.argtypes = [P(vp), i]
    L.kd_destroy.argtypes = [vp]
    L.kd_commit_vertices_device.argtypes = [vp, vp, i, i, vp, vp, vp]
    L.kd_commit_edges_device.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp]
    L.kd_get_info.argtypes = [vp, P(i), P(i), P(i)]
    L.kd_set_timing.argtypes = [vp, i]
    L.kd_num_kernels.restype = i
    L.kd_kernel_name.restype = C.c_char_p
    L.kd_kernel_name.argtypes = [i]
    L.kd_get_kernel_times.argtypes = [vp, vp, vp, i]
    L._kd_declared = True


class GraphEdits(TimedStage):
    """Scratch for `max_rows` edit rows per call: intake records for commit_vertices_device, jobs * max_links link
    records for commit_edges_device."""

    _PREFIX = "kd"

    def __init__(self, max_rows: int):
        self.L = library(_declare)
        self.max_rows = int(max_rows)
        self.h = C.c_void_p()
        self._check(self.L.kd_create(C.byref(self.h), self.max_rows), "kd_create")

    def commit_vertices_device(self, d_intake: int, g_first: int, count: int, loop_fleet, spa_fleet=None,
                               hip_stream: int = 0):
        """kd_commit_vertices_device on ProcessStage.result_device()'s intake records."""
        self._check(self.L.kd_commit_vertices_device(self.h, _dp(d_intake), int(g_first), int(count), loop_fleet.h,
                                                     spa_fleet.h if spa_fleet is not None else None, _dp(hip_stream)),
                    "kd_commit_vertices_device")

    def commit_edges_device(self, d_jobs_out: int, d_links: int, max_links: int, first_job: int, count: int, loop_fleet,
                            spa_fleet=None, hip_stream: int = 0):
        """kd_commit_edges_device on LinkStage.result_device()'s arrays."""
        self._check(self.L.kd_commit_edges_device(self.h, _dp(d_jobs_out), _dp(d_links), int(max_links), int(first_job),
                                                  int(count), loop_fleet.h,
                                                  spa_fleet.h if spa_fleet is not None else None, _dp(hip_stream)),
                    "kd_commit_edges_device")

    def info(self):
        """(vertices added, new edges, rows refused) since the last call; waits."""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.L.kd_get_info(self.h, C.byref(a), C.byref(b), C.byref(c)), "kd_get_info")
        return a.value, b.value, c.value
