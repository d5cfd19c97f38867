"""Karto's pose-correction stage over the MI355X C-ABI (include/slam2d/karto_correct.h).

Reference: LocalizedRangeScan::Update after SetSensorPose (lesson6/lib/open_karto/include/open_karto/Karto.h:5362-5416,
reached from Mapper.cpp:1032 and :2044) and MapperGraph::CorrectPoses (Mapper.cpp:1397-1414), applied to the
device-resident graphs of a `LoopSearchFleet`, a `SpaFleet` and up to two `ScanMatcher` pools from the device-resident
records of a `ProcessStage` and a `LinkStage`, with no count read on the host: `PoseCorrection` mirrors the kc_* entry
points one to one.  Results are checked against the per-graph host-indexed calls (kl_set_scans_device,
kt_set_scans_device, spa_compute) bit for bit.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib  # noqa: F401  (callers reach the library through the module)
from ._lib import Slam2dError  # noqa: F401
from ._stage import TimedStage, dp as _dp, hp as _hp, library
from . import karto as _kt
from . import karto_loop as _kl
from . import spa as _spa

KC_OK, KC_EINVAL, KC_EHIP, KC_ENOMEM, KC_ENODEV, KC_ERANGE = 0, -1, -2, -3, -4, -5
KC_MAX_ROWS = 4096


def _declare(L):
    if getattr(L, "_kc_declared", False):
        return
    vp, i, P = C.c_void_p, C.c_int, C.POINTER
    _kt._declare(L)
    _kl._declare(L)
    _spa._declare(L)
    L.kc_last_error.restype = C.c_char_p
    L.kc_version.restype = C.c_char_p
    L.kc_create.argtypes = [P(vp), i, i, vp, i]
    L.kc_destroy.argtypes = [vp]
    L.kc_refresh_intake_device.argtypes = [vp, vp, i, i, vp, vp, vp, vp, vp, i, vp]
    L.kc_refresh_jobs_device.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, i, vp]
    L.kc_correct_poses_device.argtypes = [vp, vp, vp, i, vp, P(_spa.SpaParams), vp, vp, vp, vp, vp, i, vp]
    L.kc_get_info.argtypes = [vp, P(i), P(i), P(i)]
    L.kc_set_timing.argtypes = [vp, i]
    L.kc_num_kernels.restype = i
    L.kc_kernel_name.restype = C.c_char_p
    L.kc_kernel_name.argtypes = [i]
    L.kc_get_kernel_times.argtypes = [vp, vp, vp, i]
    L._kc_declared = True


def _h(stage):
    return stage.h if stage is not None else None


class PoseCorrection(TimedStage):
    """`n_graphs` graphs of up to `max_scans` scans, graph g's scan i in pool slot pool_offset[g] + i (None: g *
    max_scans), and scratch rows for `max_rows` (<= KC_MAX_ROWS) records per call."""

    _PREFIX = "kc"

    def __init__(self, n_graphs: int, max_scans: int, pool_offset=None, max_rows: int = KC_MAX_ROWS):
        self.L = library(_declare)
        self.n_graphs, self.max_scans, self.max_rows = int(n_graphs), int(max_scans), int(max_rows)
        off = None if pool_offset is None else np.ascontiguousarray(pool_offset, np.int32).reshape(self.n_graphs)
        self.h = C.c_void_p()
        self._check(self.L.kc_create(C.byref(self.h), self.n_graphs, self.max_scans, _hp(off) if off is not None else None,
                                     self.max_rows), "kc_create")

    def refresh_intake_device(self, d_intake: int, g_first: int, count: int, d_pool_ranges: int, d_pool_poses: int,
                              pool_scans: int, loop_fleet=None, matcher_seq=None, matcher_loop=None, hip_stream: int = 0):
        """kc_refresh_intake_device on ProcessStage.result_device()'s intake records."""
        self._check(self.L.kc_refresh_intake_device(self.h, _dp(d_intake), int(g_first), int(count), _h(loop_fleet),
                                                    _h(matcher_seq), _h(matcher_loop), _dp(d_pool_ranges),
                                                    _dp(d_pool_poses), int(pool_scans), _dp(hip_stream)),
                    "kc_refresh_intake_device")

    def refresh_jobs_device(self, d_jobs: int, d_closures: int, count: int, d_pool_ranges: int, d_pool_poses: int,
                            pool_scans: int, loop_fleet=None, matcher_seq=None, matcher_loop=None, hip_stream: int = 0):
        """kc_refresh_jobs_device: every job row's scan, or with d_closures only where a closure was accepted."""
        self._check(self.L.kc_refresh_jobs_device(self.h, _dp(d_jobs), _dp(d_closures), int(count), _h(loop_fleet),
                                                  _h(matcher_seq), _h(matcher_loop), _dp(d_pool_ranges),
                                                  _dp(d_pool_poses), int(pool_scans), _dp(hip_stream)),
                    "kc_refresh_jobs_device")

    def correct_poses_device(self, d_jobs: int, d_closures: int, count: int, spa_fleet, d_pool_ranges: int,
                             d_pool_poses: int, pool_scans: int, params=None, loop_fleet=None, matcher_seq=None,
                             matcher_loop=None, hip_stream: int = 0):
        """kc_correct_poses_device: CorrectPoses for the graphs of the job rows whose closure was accepted."""
        p = params if params is not None else _spa.default_params()
        self._check(self.L.kc_correct_poses_device(self.h, _dp(d_jobs), _dp(d_closures), int(count), spa_fleet.h,
                                                   C.byref(p), _h(loop_fleet), _h(matcher_seq), _h(matcher_loop),
                                                   _dp(d_pool_ranges), _dp(d_pool_poses), int(pool_scans),
                                                   _dp(hip_stream)), "kc_correct_poses_device")

    def info(self):
        """(scans the refresh records named, records whose graph was corrected, records refused) since the last
        call; waits."""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.L.kc_get_info(self.h, C.byref(a), C.byref(b), C.byref(c)), "kc_get_info")
        return a.value, b.value, c.value
