"""Lidar motion undistortion (lesson5) over the MI355X C-ABI (include/slam2d/undistort.h).

Reference: lesson5/src/lidar_undistortion.cc.
  * UndistortFleet     the ud_* entry points: a batch of scans, their IMU windows and odometry pairs in device
                       memory -> the corrected cloud and Hector DataContainer points (HectorFleet.step_device's
                       layout), one kernel launch.  There is no CPU path here.
  * LidarUndistortion  the node's host side with the reference's method names: the message deques, the two-scan
                       cache (CacheLaserScan :127-159), both prunes (:177-200, :252-296).  prepare() is pure
                       Python and returns the one-scan record the kernel takes; ScanCallback hands it to a fleet.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import deque

import numpy as np

from . import _lib
from ._stage import Stage, dp, hp
from .hector import HsLaser

UD_SCAN_OK, UD_SCAN_WAIT_IMU, UD_SCAN_WAIT_ODOM = 0, 1, 2
UD_MAX_IMU = 2000  # queueLength, lidar_undistortion.cc:20

_f, _i, _p, _d = C.c_float, C.c_int, C.c_void_p, C.c_double
_declared = False


def _L():
    global _declared
    L = _lib.lib()
    if not _declared:
        P = C.POINTER
        L.ud_version.restype = C.c_char_p
        L.ud_last_error.restype = C.c_char_p
        L.ud_create.argtypes = [P(_p), _i, _i, _i]
        L.ud_destroy.argtypes = [_p]
        L.ud_set_scan_geometry.argtypes = [_p, _f, _f, _f, _f, _p]
        L.ud_default_laser.restype = None
        L.ud_default_laser.argtypes = [_p, _i, _f, _f]
        L.ud_set_container_rules.argtypes = [_p, _p, _f]
        L.ud_set_sources.argtypes = [_p, _i, _i]
        L.ud_correct_batch_device.argtypes = [_p, _i, _p, _i, _p, _p, _i, _p, _p, _p, _i, _p, _i, _p, _p, _p, _p]
        L.ud_correct.argtypes = [_p, _p, _d, _d, _p, _i, _p, _p, _p, P(_i), _p, P(_i)]
        L.ud_rpy_from_quaternion.argtypes = [_p, _p]
        L.ud_get_stream.restype = _p
        L.ud_get_stream.argtypes = [_p]
        _declared = True
    return L


def _dev(x):
    """A device address from an int, a torch tensor (data_ptr) or None."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x) or None)


def rpy_from_quaternion(q) -> np.ndarray:
    """tf::Matrix3x3(q).getRPY of q = (x, y, z, w) through the library (ud_rpy_from_quaternion)."""
    qa = np.ascontiguousarray(q, np.float64).reshape(4)
    out = np.zeros(3, np.float64)
    ud = UndistortFleet.__new__(UndistortFleet)  # the call takes no context: the library and the prefix are enough
    ud.L = _L()
    ud._check(ud.L.ud_rpy_from_quaternion(hp(qa), hp(out)), "ud_rpy_from_quaternion")
    return out


def default_laser(n_beams: int, angle_min: float = 0.0, angle_increment: float = 0.0) -> HsLaser:
    """ud_default_laser: hs_default_laser with the z window (0, 2) -- the corrected cloud sits at z = 1."""
    laser = HsLaser()
    _L().ud_default_laser(C.byref(laser), int(n_beams), angle_min, angle_increment)
    return laser


class UndistortFleet(Stage):
    """num_streams scanners of n_beams ranges each (ud_ctx)."""

    _PREFIX = "ud"

    def __init__(self, num_streams: int = 1, n_beams: int = 1081, max_imu: int = UD_MAX_IMU):
        self.L = _L()
        self.B, self.n, self.max_imu = int(num_streams), int(n_beams), int(max_imu)
        h = C.c_void_p()
        self._check(self.L.ud_create(C.byref(h), self.B, self.n, self.max_imu), "ud_create")
        self.h = h

    def set_scan_geometry(self, angle_min: float, angle_increment: float, range_min: float, range_max: float,
                          unit_vectors=None):
        """The LaserScan fields the node reads; unit_vectors [n, 2] double or None (CreateAngleCache, host libm)."""
        uv = None
        if unit_vectors is not None:
            uv = np.ascontiguousarray(unit_vectors, np.float64).reshape(-1)
            if uv.size != 2 * self.n:
                raise ValueError("unit_vectors must be [n_beams, 2]")
        self._check(self.L.ud_set_scan_geometry(self.h, angle_min, angle_increment, range_min, range_max,
                                                hp(uv) if uv is not None else None), "ud_set_scan_geometry")

    def set_container_rules(self, laser: HsLaser, scale_to_map: float):
        self._check(self.L.ud_set_container_rules(self.h, C.byref(laser), scale_to_map), "ud_set_container_rules")

    def set_sources(self, use_imu: bool, use_odom: bool):
        self._check(self.L.ud_set_sources(self.h, int(bool(use_imu)), int(bool(use_odom))), "ud_set_sources")

    def stream_handle(self) -> int:
        return int(self.L.ud_get_stream(self.h) or 0)

    def correct_device(self, count: int, d_ranges, range_stride: int, d_scan_time, d_imu=None, imu_stride: int = 0,
                       d_imu_n=None, d_odom=None, d_cloud=None, cloud_stride: int = 0, d_xy=None, xy_stride: int = 0,
                       d_n=None, d_origo=None, d_status=None, hip_stream: int = 0):
        """ud_correct_batch_device; every buffer is a device address (int) or a torch tensor, outputs may be None."""
        self._check(self.L.ud_correct_batch_device(self.h, int(count), _dev(d_ranges), int(range_stride),
                                                   _dev(d_scan_time), _dev(d_imu), int(imu_stride), _dev(d_imu_n),
                                                   _dev(d_odom), _dev(d_cloud), int(cloud_stride), _dev(d_xy),
                                                   int(xy_stride), _dev(d_n), _dev(d_origo), _dev(d_status),
                                                   dp(hip_stream)), "ud_correct_batch_device")

    def correct(self, ranges, scan_time_start: float, scan_time_increment: float, imu=None, odom=None) -> dict:
        """ud_correct: one scan from host arrays.  imu [k, 4] (t, wx, wy, wz), odom [2, 7]
        (t, x, y, z, roll, pitch, yaw).  Returns status, cloud [n, 3], xy [m, 2] (map scale), origo."""
        r = np.ascontiguousarray(ranges, np.float32)
        if r.size != self.n:
            raise ValueError("ranges must hold n_beams values")
        im = np.ascontiguousarray(imu, np.float64).reshape(-1, 4) if imu is not None else np.zeros((0, 4))
        od = np.ascontiguousarray(odom, np.float64).reshape(2, 7) if odom is not None else None
        cloud = np.zeros((self.n, 3), np.float32)
        xy = np.zeros((self.n, 2), np.float32)
        origo = np.zeros(2, np.float32)
        n, st = C.c_int(), C.c_int()
        self._check(self.L.ud_correct(self.h, hp(r), scan_time_start, scan_time_increment, hp(im) if len(im) else None,
                                      len(im), hp(od) if od is not None else None, hp(cloud), hp(xy), C.byref(n),
                                      hp(origo), C.byref(st)), "ud_correct")
        return {"status": st.value, "cloud": cloud, "xy": xy[: n.value].copy(), "n": n.value, "origo": origo}


def _rpy(q) -> tuple:
    """tf::Matrix3x3(q).getRPY (setRotation + getEulerYPR, solution 1) in Python doubles (:308-309)."""
    x, y, z, w = (float(v) for v in q)
    d = x * x + y * y + z * z + w * w
    s = 2.0 / d
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    m00, m01, m02 = 1.0 - (yy + zz), xy - wz, xz + wy
    m10 = xy + wz
    m20, m21, m22 = xz - wy, yz + wx, 1.0 - (xx + yy)
    if abs(m20) >= 1.0:
        if m20 < 0.0:
            return math.atan2(m01, m02), math.pi / 2.0, 0.0
        return math.atan2(-m01, -m02), -math.pi / 2.0, 0.0
    pitch = -math.asin(m20)
    c = math.cos(pitch)
    return math.atan2(m21 / c, m22 / c), pitch, math.atan2(m10 / c, m00 / c)


class LidarUndistortion:
    """Host mirror of the node (lesson5/src/lidar_undistortion.cc:22-159, 177-200, 252-296).

    Messages are plain values: ImuCallback(stamp, angular_velocity), OdomCallback(stamp, position, orientation
    (x, y, z, w)), ScanCallback(stamp, time_increment, ranges); stamps are seconds (header.stamp.toSec())."""

    def __init__(self, fleet: UndistortFleet | None = None, use_imu: bool = True, use_odom: bool = True):
        self.fleet = fleet
        self.use_imu_, self.use_odom_ = bool(use_imu), bool(use_odom)  # :27-28
        self.imu_queue_: deque = deque()
        self.odom_queue_: deque = deque()
        self.laser_queue_: deque = deque()
        self.first_scan_ = True  # :48
        self.scan_count_ = 0
        self.start_odom_msg_ = None  # members of the node: they persist from scan to scan (:286, :292)
        self.end_odom_msg_ = None
        if fleet is not None:
            fleet.set_sources(self.use_imu_, self.use_odom_)

    def ImuCallback(self, stamp: float, angular_velocity):  # :82-86
        wx, wy, wz = (float(v) for v in angular_velocity)
        self.imu_queue_.append((float(stamp), wx, wy, wz))

    def OdomCallback(self, stamp: float, position, orientation):  # :89-93
        self.odom_queue_.append((float(stamp), tuple(float(v) for v in position), tuple(float(v) for v in orientation)))

    def prepare(self, stamp: float, time_increment: float, ranges):
        """CacheLaserScan, PruneImuDeque's and PruneOdomDeque's queue handling for one LaserScan, without the GPU.
        None while the scan is only cached (:145-146); else the record of the scan that left the cache:
        status (UD_SCAN_*), ranges, scan_time (start, increment), imu [k, 4], odom [2, 7]."""
        r = np.ascontiguousarray(ranges, np.float32)
        if self.first_scan_:  # :129-137
            self.first_scan_ = False
            self.scan_count_ = r.size
        self.laser_queue_.append((float(stamp), float(np.float32(time_increment)), r))  # :142
        if len(self.laser_queue_) < 2:  # :145-146
            return None
        start, inc, cur = self.laser_queue_.popleft()  # :149-155
        end = start + inc * (float(self.scan_count_) - 1)  # :156
        rec = {"status": UD_SCAN_OK, "ranges": cur, "scan_time": (start, inc), "scan_time_end": end,
               "imu": np.zeros((0, 4), np.float64), "odom": np.full((2, 7), np.nan, np.float64)}
        if self.use_imu_:  # :103-107
            q = self.imu_queue_
            if not q or q[0][0] > start or q[-1][0] < end:  # :182-188
                rec["status"] = UD_SCAN_WAIT_IMU
                return rec
            while q and q[0][0] < start - 0.1:  # :191-197
                q.popleft()
            if not q:  # :199-200
                rec["status"] = UD_SCAN_WAIT_IMU
                return rec
            win = []
            for s in q:  # the loop of :207-243 stops at the first sample after the scan end
                win.append(s)
                if s[0] > end:
                    break
            rec["imu"] = np.asarray(win, np.float64).reshape(-1, 4)
            if not (win[0][0] < start) or len(win) > UD_MAX_IMU:  # the node would index imu_time_ out of range
                rec["status"] = UD_SCAN_WAIT_IMU
                return rec
        if self.use_odom_:  # :110-114
            q = self.odom_queue_
            if not q or q[0][0] > start or q[-1][0] < end:  # :257-263
                rec["status"] = UD_SCAN_WAIT_ODOM
                return rec
            while q and q[0][0] < start - 0.1:  # :266-272
                q.popleft()
            if not q:  # :274-275
                rec["status"] = UD_SCAN_WAIT_ODOM
                return rec
            for m in q:  # :280-296
                if m[0] < start:
                    self.start_odom_msg_ = m
                    continue
                if m[0] <= end:
                    self.end_odom_msg_ = m
                else:
                    break
            if self.start_odom_msg_ is None or self.end_odom_msg_ is None:
                # (the node would go on with a default-constructed message; here: no covering pair)
                rec["status"] = UD_SCAN_WAIT_ODOM
                return rec
            for k, m in enumerate((self.start_odom_msg_, self.end_odom_msg_)):  # :301-325
                rec["odom"][k] = (m[0],) + m[1] + _rpy(m[2])
        return rec

    def ScanCallback(self, stamp: float, time_increment: float, ranges):  # :96-124
        """The corrected scan that left the two-scan cache: the record of prepare() plus cloud, xy, n, origo
        (UndistortFleet.correct); None while caching; the bare record (status != 0) while waiting."""
        rec = self.prepare(stamp, time_increment, ranges)
        if rec is None or rec["status"] != UD_SCAN_OK:
            return rec
        if self.fleet is None:
            raise _lib.Slam2dError("LidarUndistortion.ScanCallback needs an UndistortFleet")
        out = self.fleet.correct(rec["ranges"], rec["scan_time"][0], rec["scan_time"][1],
                                 rec["imu"] if self.use_imu_ else None, rec["odom"] if self.use_odom_ else None)
        rec.update(out)
        return rec
