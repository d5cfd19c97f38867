"""The lesson5 lidar undistortion without a GPU: the CPU restatement (tests/ref/undistort_ref.c) against its
golden fixture and against physics, the host mirror's queue handling (LidarUndistortion.prepare), and
ud_rpy_from_quaternion.  The GPU parity of the kernel against the same restatement is tests/test_undistort_gpu.py.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import undistort_ref as R  # noqa: E402

from slam2d import synth  # noqa: E402
from slam2d.undistort import (UD_SCAN_OK, UD_SCAN_WAIT_IMU, UD_SCAN_WAIT_ODOM, LidarUndistortion,  # noqa: E402
                              rpy_from_quaternion)


# ---------------------------------------------------------------- the restatement against its fixture
def test_restatement_reproduces_golden_fixture():
    cases = R.load_golden()
    assert [n for n, _ in R.golden_specs()] == list(cases)
    seen = set()
    for name, (c, want) in cases.items():
        assert c["n"] == R.GOLDEN_N
        got = R.correct(c)
        assert got["status"] == want["status"], name
        assert got["n"] == want["n"], name
        assert R.bits_equal(got["cloud"], want["cloud"]), name
        assert R.bits_equal(got["xy"], want["xy"]), name
        assert R.bits_equal(got["origo"], want["origo"]), name
        seen.add(want["status"])
    assert seen == {UD_SCAN_OK, UD_SCAN_WAIT_IMU, UD_SCAN_WAIT_ODOM}


def test_restatement_plain_projection_without_sources():
    """use_imu and use_odom off: transBt is the identity, the cloud is the polar projection at z = 1 (:343, :361-362)."""
    c = R.make_case(257, 21, use_imu=False, use_odom=False)
    got = R.correct(c)
    r = c["ranges"]
    ok = np.isfinite(r) & ~(r < np.float32(c["range_min"])) & ~(r > np.float32(c["range_max"]))
    want = np.zeros((257, 3), np.float32)
    want[ok, 0] = (r[ok].astype(np.float64) * c["cs"][ok, 0]).astype(np.float32)
    want[ok, 1] = (r[ok].astype(np.float64) * c["cs"][ok, 1]).astype(np.float32)
    want[ok, 2] = 1.0
    assert got["status"] == 0 and 0 < ok.sum() < 257
    assert R.bits_equal(got["cloud"], want)


# ---------------------------------------------------------------- the restatement against physics
N_PHYS = 360
SWEEP = 0.1                 # seconds per sweep
POSE0 = (6.0, 3.5, 0.4)     # room-frame pose of the scanner at the scan start
# Measured with this file on the CPU (x86-64, gcc -O2 -ffp-contract=off), noise-free, 360 beams:
#   (a) pure rotation     max residual of the corrected cloud 1.75e-06 m
#   (b) pure translation  max residual of the corrected cloud 9.29e-07 m
# The residual is float rounding (the ranges and the cloud are float32: half an ulp of a 17 m coordinate is
# 9.5e-7 m) and varies with the geometry, so the test allows 4 x the larger measured value.
MEASURED_MAX_RESIDUAL = 1.75e-06
RESIDUAL_TOL = 4.0 * MEASURED_MAX_RESIDUAL


def _seg_dist(p, segs):
    """Distance of every point [m, 2] to its nearest wall segment."""
    a, b = segs[:, 0, :], segs[:, 1, :]
    e = b - a
    w = p[:, None, :] - a[None, :, :]
    u = np.clip((w * e[None]).sum(-1) / (e * e).sum(-1)[None], 0.0, 1.0)
    d = w - u[..., None] * e[None]
    return np.sqrt((d * d).sum(-1)).min(axis=1)


def _physical_case(omega, vel):
    """A sweep cast beam by beam from the pose the scanner has at each beam's time: constant yaw rate omega
    (rad/s) and constant room-frame velocity vel (m/s).  Returns the restatement's case, the start pose."""
    n = N_PHYS
    segs = synth.world_segments()
    t_start, t_inc = 1000.0, float(np.float32(SWEEP / n))
    ti = t_start + np.arange(n) * t_inc
    dt = ti - t_start
    poses = np.stack([POSE0[0] + vel[0] * dt, POSE0[1] + vel[1] * dt, POSE0[2] + omega * dt], axis=1)
    full = synth.cast_ranges(poses, segs, n)      # [n poses, n beams]
    ranges = np.diagonal(full).astype(np.float32)  # beam i from pose i
    ang = synth.beam_angles(n)
    cs = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    # IMU at 200 Hz straddling the sweep, one sample exactly at the scan end: the reference holds the rotation of
    # the last in-window sample for later beams (:414-419, "can only approximate"), which at 200 Hz and 1.2 rad/s
    # costs up to 6.1e-03 m on the last beams (measured with a grid whose last in-window sample is 2 ms before the
    # end); with a sample at the end
    # every beam is interpolated.  Odometry records before the start and inside the sweep.
    t_end = t_start + t_inc * (float(n) - 1)
    timu = t_end + 0.005 * np.arange(-23, 3)
    imu = np.stack([timu, np.zeros_like(timu), np.zeros_like(timu), np.full_like(timu, omega)], axis=1)
    odom = np.zeros((2, 7))
    for k, to in enumerate((t_start - 0.02, t_start + 0.07)):
        d = to - t_start
        odom[k] = (to, POSE0[0] + vel[0] * d, POSE0[1] + vel[1] * d, 0.0, 0.0, 0.0, POSE0[2] + omega * d)
    case = {"n": n, "ranges": ranges, "cs": cs, "range_min": 0.1, "range_max": 30.0, "t_start": t_start,
            "t_inc": t_inc, "use_imu": omega != 0.0, "use_odom": any(v != 0.0 for v in vel), "imu": imu, "odom": odom,
            "rules": dict(R.DEFAULT_RULES), "scale": 20.0}
    return case, segs, cs


def _residuals(case, segs, cs):
    """Per valid beam: distance to the walls of the corrected point and of the uncorrected polar projection, both
    mapped into the room by the pose at the scan's first valid beam (beam 0 here)."""
    got = R.correct(case)
    assert got["status"] == 0
    valid = np.isfinite(case["ranges"])
    assert valid[0] and valid.sum() > N_PHYS // 2
    c, s = math.cos(POSE0[2]), math.sin(POSE0[2])
    rot = np.array([[c, -s], [s, c]])

    def to_room(xy):
        return xy @ rot.T + np.asarray(POSE0[:2])

    corrected = got["cloud"][valid, :2].astype(np.float64)
    assert np.all(np.abs(got["cloud"][valid, 2] - 1.0) < 1e-6)  # planar motion keeps the reference's z = 1
    raw = case["ranges"][valid, None].astype(np.float64) * cs[valid]
    return _seg_dist(to_room(corrected), segs), _seg_dist(to_room(raw), segs)


@pytest.mark.parametrize("name,omega,vel", [("rotation", 1.2, (0.0, 0.0)), ("translation", 0.0, (1.1, -0.6))])
def test_restatement_is_physically_right(name, omega, vel):
    """(a) pure rotation at a constant rate with IMU samples straddling the sweep, (b) pure translation at a
    constant velocity with odometry: every corrected point, mapped by the start pose, lies on its wall within
    RESIDUAL_TOL = 7.0e-06 m = 4 x the measured maximum 1.75e-06 m ((a) 1.75e-06 m, (b) 9.29e-07 m; float
    rounding, see above), while the uncorrected projection misses by more than that on at least half of the
    valid beams (else the case would prove nothing)."""
    case, segs, cs = _physical_case(omega, vel)
    res, raw = _residuals(case, segs, cs)
    print(f"{name}: corrected max {res.max():.3e} m, uncorrected max {raw.max():.3e} m, "
          f"uncorrected beyond tol {np.mean(raw > RESIDUAL_TOL):.2f} of {len(raw)} beams")
    assert np.mean(raw > RESIDUAL_TOL) >= 0.5
    assert res.max() < RESIDUAL_TOL


def test_restatement_combined_motion_is_recorded():
    """Rotation and translation together: recorded, not asserted -- the reference interpolates the position along
    the straight odometry increment in the START odom frame while the scanner turns, which is inexact (measured
    here: max residual 3.57e-04 m at 1.2 rad/s and 1.25 m/s, against 9.6e-01 m uncorrected)."""
    case, segs, cs = _physical_case(1.2, (1.1, -0.6))
    res, raw = _residuals(case, segs, cs)
    print(f"combined: corrected max {res.max():.3e} m, uncorrected max {raw.max():.3e} m")
    assert np.isfinite(res).all()


# ---------------------------------------------------------------- LidarUndistortion.prepare on hand-built queues
Q_ID = (0.0, 0.0, 0.0, 1.0)


def _node(**kw):
    return LidarUndistortion(None, **kw)


def _scan(n=11):
    return np.full(n, 2.0, np.float32)


def test_prepare_first_scan_is_only_cached():
    u = _node()
    assert u.prepare(10.0, 0.01, _scan()) is None                      # :145-146
    assert len(u.laser_queue_) == 1 and u.scan_count_ == 11


def test_prepare_waits_for_imu_until_the_scan_end_is_covered():
    u = _node(use_odom=False)
    u.prepare(10.0, 0.01, _scan())                                    # scan A: 10.0 .. 10.1
    for t in (9.95, 10.0, 10.05):
        u.ImuCallback(t, (0.0, 0.0, 0.5))
    rec = u.prepare(10.2, 0.01, _scan())                               # A leaves the cache; IMU ends at 10.05
    assert rec["status"] == UD_SCAN_WAIT_IMU and rec["scan_time"] == (10.0, float(np.float32(0.01)))
    assert len(u.imu_queue_) == 3                                      # :182-188 returns before the trimming
    for t in (10.1, 10.15, 10.2, 10.25, 10.31):
        u.ImuCallback(t, (0.0, 0.0, 0.5))
    rec = u.prepare(10.4, 0.01, _scan())                               # scan B: 10.2 .. 10.3
    assert rec["status"] == UD_SCAN_OK and rec["scan_time"][0] == 10.2
    # trimmed at start - 0.1 (:191-197): 9.95, 10.0, 10.05 are gone; the window stops at the first sample after the end
    assert [s[0] for s in u.imu_queue_][0] == 10.1
    assert rec["imu"][:, 0].tolist() == [10.1, 10.15, 10.2, 10.25, 10.31]
    assert rec["imu"][0, 3] == 0.5


def test_prepare_imu_front_after_scan_start_waits():
    u = _node(use_odom=False)
    u.prepare(10.0, 0.01, _scan())
    for t in (10.01, 10.2):
        u.ImuCallback(t, (0.0, 0.0, 0.0))
    assert u.prepare(10.2, 0.01, _scan())["status"] == UD_SCAN_WAIT_IMU   # :183


def test_prepare_odom_front_after_scan_start_waits():
    u = _node(use_imu=False)
    u.prepare(10.0, 0.01, _scan())
    u.OdomCallback(10.02, (0.0, 0.0, 0.0), Q_ID)
    u.OdomCallback(10.3, (0.0, 0.0, 0.0), Q_ID)
    rec = u.prepare(10.2, 0.01, _scan())
    assert rec["status"] == UD_SCAN_WAIT_ODOM and np.isnan(rec["odom"][:, 0]).all()   # :258


def test_prepare_picks_start_and_end_odom_and_trims():
    u = _node(use_imu=False)
    u.prepare(10.0, 0.01, _scan())                                    # 10.0 .. 10.1
    yaw = 0.3
    q = (0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2))
    for t in (9.85, 9.92, 9.97, 10.0, 10.04, 10.09, 10.13, 10.2):
        u.OdomCallback(t, (t, 2.0 * t, 0.0), q)
    rec = u.prepare(10.2, 0.01, _scan())
    assert rec["status"] == UD_SCAN_OK
    assert u.odom_queue_[0][0] == 9.92                                 # 9.85 < start - 0.1 is trimmed (:266-272)
    # start = the last record before the scan start, end = the last one <= the scan end (:280-296)
    assert rec["odom"][0, 0] == 9.97 and rec["odom"][1, 0] == 10.09
    assert rec["odom"][1, 1:4].tolist() == [10.09, 2.0 * 10.09, 0.0]
    np.testing.assert_allclose(rec["odom"][0, 4:], [0.0, 0.0, yaw], atol=1e-15)


def test_prepare_needs_no_gpu_and_scancallback_needs_a_fleet():
    u = _node(use_imu=False, use_odom=False)
    assert u.ScanCallback(1.0, 0.001, _scan()) is None
    with pytest.raises(Exception, match="UndistortFleet"):
        u.ScanCallback(1.2, 0.001, _scan())


# ---------------------------------------------------------------- ud_rpy_from_quaternion
def test_rpy_from_quaternion_hand_values():
    assert rpy_from_quaternion((0.0, 0.0, 0.0, 1.0)).tolist() == [0.0, 0.0, 0.0]
    h = math.sqrt(0.5)
    np.testing.assert_allclose(rpy_from_quaternion((0.0, 0.0, h, h)), [0.0, 0.0, math.pi / 2], atol=1e-15)
    # roll 0.1, pitch -0.2, yaw 0.3 composed as Rz(yaw) Ry(pitch) Rx(roll) (tf's setRPY convention)
    r, p, y = 0.1, -0.2, 0.3
    cr, sr, cp, sp, cy, sy = (math.cos(r / 2), math.sin(r / 2), math.cos(p / 2), math.sin(p / 2), math.cos(y / 2),
                              math.sin(y / 2))
    q = (sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
         cr * cp * cy + sr * sp * sy)
    np.testing.assert_allclose(rpy_from_quaternion(q), [r, p, y], atol=1e-15)
    # a quaternion that is not normalised gives the same angles (setRotation divides by length2)
    np.testing.assert_allclose(rpy_from_quaternion(tuple(3.0 * v for v in q)), [r, p, y], atol=1e-15)
    # the host mirror's pure-Python getRPY (LidarUndistortion.prepare) is the same sequence of double operations
    from slam2d.undistort import _rpy
    rng = np.random.default_rng(8)
    for qq in rng.normal(size=(50, 4)):
        assert tuple(rpy_from_quaternion(qq)) == _rpy(qq)
    # gimbal lock: pitch = +pi/2, yaw reported as 0
    out = rpy_from_quaternion((0.0, h, 0.0, h))
    assert out[2] == 0.0 and abs(out[1] - math.pi / 2) < 1e-15
