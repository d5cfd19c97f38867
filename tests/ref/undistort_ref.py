"""ctypes loader of tests/ref/undistort_ref.c (the CPU restatement of lesson5's LidarUndistortion) and the
input cases the undistortion tests share.  Test infrastructure: nothing here is imported by the package.

The restatement is built on demand with `gcc -O2 -ffp-contract=off` into a temporary directory (no build
product lands in the tree); it includes csrc/detmath.h for the float sin / cos.
"""
from __future__ import annotations

import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(REPO, "creating-2d-laser-slam-from-scratch_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "undistort_cases.npz")

_LIB = None

# ud_default_laser's DataContainer rules (hs_default_laser, hector_slam.cc:129, 151-161, with the z window (0, 2)),
# in the form oracle.ingest's dict has them
DEFAULT_RULES = {"tf": [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], "use_max": 20.0,
                 "sqr_min": float(np.float32(0.2 * 0.2)), "sqr_max": float(np.float32(30.0 * 30.0)),
                 "z_min": 0.0, "z_max": 2.0}
# a pitched, offset laser with a narrow z window and a negative lower distance bound (the cloud's zero points
# of invalid beams then pass :336 and reach the z test)
TILTED_RULES = {"tf": [float(np.cos(0.08)), 0.0, float(np.sin(0.08)), 0.0, 1.0, 0.0, -float(np.sin(0.08)), 0.0,
                       float(np.cos(0.08)), 0.31, -0.07, 0.4], "use_max": 18.0, "sqr_min": -1.0,
                "sqr_max": float(np.float32(25.0 * 25.0)), "z_min": -0.2, "z_max": 1.6}


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        td = tempfile.mkdtemp(prefix="undistort_ref_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "libundistort_ref.so")
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-std=c99", "-shared", "-fPIC", "-I", CSRC,
                        os.path.join(HERE, "undistort_ref.c"), "-o", so, "-lm"], check=True)
        L = C.CDLL(so)
        p, i, f, d = C.c_void_p, C.c_int, C.c_float, C.c_double
        L.udr_unit_vectors.restype = None
        L.udr_unit_vectors.argtypes = [i, f, f, p]
        L.udr_correct.restype = i
        L.udr_correct.argtypes = [i, p, p, f, f, d, d, i, p, i, i, p, p, p, p, p, C.POINTER(i), p]
        _LIB = L
    return _LIB


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def unit_vectors(n: int, angle_min: float, angle_increment: float) -> np.ndarray:
    """CreateAngleCache (lidar_undistortion.cc:162-174): [n, 2] doubles (cos, sin)."""
    cs = np.zeros((n, 2), np.float64)
    lib().udr_unit_vectors(n, angle_min, angle_increment, _hp(cs))
    return cs


def correct(case: dict) -> dict:
    """One ScanCallback of the restatement on a case (see make_case): status, cloud [n, 3], xy [m, 2], n, origo."""
    n = int(case["n"])
    r = np.ascontiguousarray(case["ranges"], np.float32)
    cs = np.ascontiguousarray(case["cs"], np.float64)
    imu = np.ascontiguousarray(case["imu"], np.float64).reshape(-1, 4)
    odom = np.ascontiguousarray(case["odom"], np.float64).reshape(2, 7)
    ru = case["rules"]
    rules = np.asarray(list(ru["tf"]) + [ru["use_max"]], np.float64)
    frules = np.asarray([ru["sqr_min"], ru["sqr_max"], ru["z_min"], ru["z_max"], case["scale"]], np.float32)
    cloud = np.full((n, 3), -9.0, np.float32)
    xy = np.zeros((n, 2), np.float32)
    origo = np.zeros(2, np.float32)
    cnt = C.c_int(-1)
    imu_arg = imu if len(imu) else np.zeros((1, 4), np.float64)
    st = lib().udr_correct(n, _hp(r), _hp(cs), float(case["range_min"]), float(case["range_max"]),
                           float(case["t_start"]), float(case["t_inc"]), int(case["use_imu"]), _hp(imu_arg), len(imu),
                           int(case["use_odom"]), _hp(odom), _hp(rules), _hp(frules), _hp(cloud), _hp(xy),
                           C.byref(cnt), _hp(origo))
    return {"status": st, "cloud": cloud, "xy": xy[: cnt.value].copy(), "n": cnt.value, "origo": origo}


AMIN = float(np.float32(-np.pi))
RANGE_MIN, RANGE_MAX = 0.15, 20.0


def make_case(n: int, seed: int, n_imu: int = 37, first_valid: int = 0, use_imu: bool = True, use_odom: bool = True,
              imu_mode: str = "straddle", odom_mode: str = "pair", all_invalid: bool = False, rules=None,
              scale: float = 20.0) -> dict:
    """A synthetic scan with its IMU window and odometry pair.
    imu_mode: straddle  one or two samples before the scan start, one after its end, the rest inside
              hit       as straddle, and three samples sit exactly on point times (the strict < of :408)
              early_end the in-window samples stop at 40 % of the sweep (the > branch of :414 for later beams)
              at_start  the first sample is exactly at the scan start (status 1)
              late      the first sample is after the scan start (:183, status 1)
              short     the last sample is before the scan end (:184, status 1)
    odom_mode: pair, equal (start and end record at the same time: IEEE inf / NaN), none (NaN time: status 2)"""
    rng = np.random.default_rng(seed)
    ainc = float(np.float32(2.0 * np.pi / max(n, 2)))
    t_inc = float(np.float32(0.1 / n))
    t_start = 1.7e9 + float(rng.uniform(0.0, 100.0))
    t_end = t_start + t_inc * (float(n) - 1)
    span = max(t_end - t_start, 1e-4)
    r = rng.uniform(0.3, 19.0, n).astype(np.float32)
    pick = rng.integers(0, 12, n)
    r[pick == 0] = np.nan
    r[pick == 1] = np.inf
    r[pick == 2] = -np.inf
    r[pick == 3] = np.float32(0.1)      # below range_min
    r[pick == 4] = np.float32(22.0)     # above range_max
    r[pick == 5] = rng.uniform(0.15, 0.25, int((pick == 5).sum())).astype(np.float32)  # around laser_min_dist
    r[pick == 6] = rng.uniform(0.6, 0.8, int((pick == 6).sum())).astype(np.float32)    # the x < 0 && d^2 < 0.5 cut
    r[pick == 7] = np.float32(RANGE_MIN)  # exactly the bounds: kept (:351-352 are strict)
    if n > 3:
        r[n - 2] = np.float32(RANGE_MAX)
    if all_invalid:
        r[:] = np.where(np.arange(n) % 2 == 0, np.nan, 0.05).astype(np.float32)
    else:
        r[:first_valid] = np.nan
        r[first_valid] = np.float32(5.0)
    # IMU window
    k = max(n_imu, 0)
    t = np.zeros(k)
    if k >= 1:
        t[0] = t_start - 0.031
    if k >= 2:
        t[-1] = t_end + 0.004
    if k >= 3:
        inner = np.sort(rng.uniform(t_start, t_end if imu_mode != "early_end" else t_start + 0.4 * span, k - 2))
        t[1:-1] = inner
        if k >= 6:
            t[1] = t_start - 0.012  # a second sample before the start: skipped by :215
            t[2] = t_start          # exactly at the start: integrated (:212 is strict)
        if imu_mode == "hit" and n >= 8 and k >= 9:
            for j, beam in zip((4, 5, 6), (n // 4, n // 2, n - 1)):
                t[j] = t_start + beam * t_inc
            t[1:-1] = np.sort(t[1:-1])
    if imu_mode == "at_start" and k >= 1:
        t[t < t_start] = t_start
    if imu_mode == "late" and k >= 1:
        t[t < t_start + 0.25 * span] = t_start + 0.25 * span
    if imu_mode == "short" and k >= 2:
        t[-1] = t_start + 0.5 * span
        t = np.sort(t)
    imu = np.concatenate([t[:, None], rng.uniform(-1.5, 1.5, (k, 3))], axis=1)
    # odometry pair (t, x, y, z, roll, pitch, yaw)
    o0 = np.concatenate([[t_start - 0.013], rng.uniform(-5.0, 5.0, 3), rng.uniform(-0.05, 0.05, 2),
                         rng.uniform(-np.pi, np.pi, 1)])
    o1 = o0 + np.concatenate([[0.0], rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.01, 0.01, 2), rng.uniform(-0.1, 0.1, 1)])
    o1[0] = t_start + 0.8 * span
    if odom_mode == "equal":
        o1[0] = o0[0]
    if odom_mode == "none":
        o0[0] = np.nan
    cs = unit_vectors(n, AMIN, ainc)
    return {"n": n, "ranges": r, "cs": cs, "range_min": RANGE_MIN, "range_max": RANGE_MAX, "t_start": t_start,
            "t_inc": t_inc, "use_imu": bool(use_imu), "use_odom": bool(use_odom), "imu": imu,
            "odom": np.stack([o0, o1]), "rules": dict(rules or DEFAULT_RULES), "scale": float(scale)}


GOLDEN_N = 360


def golden_specs():
    """(name, make_case keyword arguments) of the fixture cases, all at 360 beams."""
    return [("default", dict(seed=1)),
            ("hit", dict(seed=2, imu_mode="hit")),
            ("early_end", dict(seed=3, imu_mode="early_end", n_imu=12)),
            ("front0", dict(seed=4, n_imu=2)),
            ("at_start", dict(seed=5, imu_mode="at_start")),
            ("no_imu", dict(seed=6, use_imu=False)),
            ("no_odom", dict(seed=7, use_odom=False)),
            ("neither", dict(seed=8, use_imu=False, use_odom=False)),
            ("equal_odom", dict(seed=9, odom_mode="equal")),
            ("wait_odom", dict(seed=10, odom_mode="none")),
            ("first300", dict(seed=11, first_valid=300)),
            ("all_invalid", dict(seed=12, all_invalid=True)),
            ("tilted", dict(seed=13, rules=TILTED_RULES, scale=10.0)),
            ("imu200", dict(seed=14, n_imu=200))]


_IN_KEYS = ("ranges", "cs", "imu", "odom")
_SCALARS = ("n", "range_min", "range_max", "t_start", "t_inc", "use_imu", "use_odom", "scale")
_RULE_KEYS = ("use_max", "sqr_min", "sqr_max", "z_min", "z_max")


def pack_golden(cases: dict) -> dict:
    """{name: (case, expected)} -> flat arrays for np.savez."""
    out = {"names": np.asarray(list(cases))}
    for name, (c, e) in cases.items():
        for k in _IN_KEYS:
            out[f"{name}/{k}"] = np.asarray(c[k])
        out[f"{name}/scalars"] = np.asarray([float(c[k]) for k in _SCALARS], np.float64)
        out[f"{name}/rules"] = np.asarray(list(c["rules"]["tf"]) + [c["rules"][k] for k in _RULE_KEYS], np.float64)
        out[f"{name}/cloud"] = e["cloud"]
        out[f"{name}/xy"] = e["xy"]
        out[f"{name}/origo"] = e["origo"]
        out[f"{name}/n_status"] = np.asarray([e["n"], e["status"]], np.int32)
    return out


def load_golden(path: str = GOLDEN) -> dict:
    """{name: (case, expected)} from tests/golden/undistort_cases.npz."""
    z = np.load(path)
    cases = {}
    for name in [str(s) for s in z["names"]]:
        sc = z[f"{name}/scalars"]
        c = {k: z[f"{name}/{k}"] for k in _IN_KEYS}
        for k, v in zip(_SCALARS, sc):
            c[k] = float(v)
        c["n"] = int(c["n"])
        c["use_imu"], c["use_odom"] = bool(c["use_imu"]), bool(c["use_odom"])
        ru = z[f"{name}/rules"]
        c["rules"] = {"tf": [float(v) for v in ru[:12]], **{k: float(v) for k, v in zip(_RULE_KEYS, ru[12:])}}
        e = {"cloud": z[f"{name}/cloud"], "xy": z[f"{name}/xy"], "origo": z[f"{name}/origo"],
             "n": int(z[f"{name}/n_status"][0]), "status": int(z[f"{name}/n_status"][1])}
        cases[name] = (c, e)
    return cases


def bits_equal(a, b) -> bool:
    """float32 arrays equal bit for bit, NaNs compared by position (their payloads may differ)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))
