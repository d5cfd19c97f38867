"""GPU parity of the lesson5 lidar undistortion (lesson5/src/lidar_undistortion.cc:96-447) as ud_correct_kernel
against the CPU restatement tests/ref/undistort_ref.c.  Bar: bit-exact -- every float bit of the corrected cloud
and of the DataContainer points, the point count, origo and the per-scan status; NaNs are compared by position.
PCL / Eigen are absent, so both sides evaluate the float pieces in the order DESIGN.md section 3 fixes (parity
unpinned against a PCL build).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import undistort_ref as R  # noqa: E402

import oracle as O  # noqa: E402
from slam2d import synth  # noqa: E402
from slam2d.hector import HectorFleet  # noqa: E402
from slam2d.undistort import LidarUndistortion, UndistortFleet, default_laser  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = -7.0


def _laser(rules):
    L = default_laser(0)
    for i, v in enumerate(rules["tf"][:9]):
        L.basis[i] = v
    for i, v in enumerate(rules["tf"][9:]):
        L.origin[i] = v
    L.sqr_laser_min_dist, L.sqr_laser_max_dist = rules["sqr_min"], rules["sqr_max"]
    L.use_max_scan_range = rules["use_max"]
    L.laser_z_min_value, L.laser_z_max_value = rules["z_min"], rules["z_max"]
    return L


def _fleet_for(cases, max_imu=None):
    c0 = cases[0]
    if max_imu is None:
        max_imu = max(1, max(len(c["imu"]) for c in cases))
    f = UndistortFleet(len(cases), c0["n"], max_imu)
    f.set_scan_geometry(0.0, 0.0, c0["range_min"], c0["range_max"], unit_vectors=c0["cs"])
    f.set_container_rules(_laser(c0["rules"]), c0["scale"])
    f.set_sources(c0["use_imu"], c0["use_odom"])
    return f


def _run(cases, want_cloud=True, want_xy=True, max_imu=None, fleet=None):
    """One ud_correct_batch_device launch over `cases` (same geometry, rules and sources); strides are wider than
    the scans and every output is poisoned, so a write out of place shows."""
    import torch

    B, n = len(cases), cases[0]["n"]
    f = fleet or _fleet_for(cases, max_imu)
    istride = max(1, max(len(c["imu"]) for c in cases)) + 1
    rs, cst, xs = n + 3, n + 1, n + 2
    ranges = np.full((B, rs), np.nan, np.float32)
    tm = np.zeros((B, 2))
    imu = np.full((B, istride, 4), np.nan)
    imu_n = np.zeros(B, np.int32)
    odom = np.zeros((B, 2, 7))
    for b, c in enumerate(cases):
        ranges[b, :n] = c["ranges"]
        tm[b] = (c["t_start"], c["t_inc"])
        imu[b, : len(c["imu"])] = c["imu"]
        imu_n[b] = len(c["imu"])
        odom[b] = c["odom"]
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    d_cloud = torch.full((B, cst, 3), POISON, dtype=torch.float32, device="cuda") if want_cloud else None
    d_xy = torch.full((B, xs, 2), POISON, dtype=torch.float32, device="cuda") if want_xy else None
    d_n = torch.full((B,), -1, dtype=torch.int32, device="cuda") if want_xy else None
    d_origo = torch.full((B, 2), POISON, dtype=torch.float32, device="cuda") if want_xy else None
    d_status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    f.correct_device(B, dev(ranges), rs, dev(tm), dev(imu), istride, dev(imu_n), dev(odom), d_cloud, cst, d_xy, xs, d_n,
                     d_origo, d_status)
    torch.cuda.synchronize()
    out = {"status": d_status.cpu().numpy()}
    if want_cloud:
        out["cloud"] = d_cloud.cpu().numpy()
    if want_xy:
        out["xy"], out["n"], out["origo"] = d_xy.cpu().numpy(), d_n.cpu().numpy(), d_origo.cpu().numpy()
    if fleet is None:
        f.close()
    return out


def _check(cases, got, wants=None):
    """Every scan of the launch against the restatement (or a stored expectation)."""
    n = cases[0]["n"]
    for b, c in enumerate(cases):
        want = wants[b] if wants else R.correct(c)
        assert got["status"][b] == want["status"], (b, got["status"][b], want["status"])
        if "cloud" in got:
            assert R.bits_equal(got["cloud"][b, :n], want["cloud"]), b
            assert np.all(got["cloud"][b, n:] == POISON), "the cloud was written past n_beams"
        if "xy" in got:
            m = want["n"]
            assert got["n"][b] == m, (b, got["n"][b], m)
            assert R.bits_equal(got["xy"][b, :m], want["xy"]), b
            assert np.all(got["xy"][b, m:] == POISON), "the DataContainer was written past its count"
            assert R.bits_equal(got["origo"][b], want["origo"]), b
    return [wants[b] if wants else R.correct(c) for b, c in enumerate(cases)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1081, 1440])
def test_scan_lengths(gpu, n):
    """Below, at and past a wave (64) and a 256-beam chunk; 1081 (Hokuyo) and 1440 (LS01B) beams."""
    cases = [R.make_case(n, 100 + n), R.make_case(n, 200 + n, n_imu=9, imu_mode="hit")]
    wants = _check(cases, _run(cases))
    assert all(w["status"] == 0 for w in wants)
    if n >= 63:
        assert 0 < wants[0]["n"] < n  # the container rules kept some beams and dropped others


def test_batch_of_five_different_windows(gpu):
    """Five scans with different IMU windows, odometry pairs and statuses in one launch (cross-scan LDS /
    indexing mix-ups would show)."""
    n = 257
    cases = [R.make_case(n, 31, n_imu=2), R.make_case(n, 32, n_imu=120, imu_mode="hit"),
             R.make_case(n, 33, n_imu=37, imu_mode="at_start"), R.make_case(n, 34, n_imu=12, imu_mode="early_end"),
             R.make_case(n, 35, n_imu=5, odom_mode="none")]
    wants = _check(cases, _run(cases))
    assert [w["status"] for w in wants] == [0, 0, 1, 0, 2]
    assert len({w["n"] for w in wants}) >= 3


@pytest.mark.parametrize("first", [0, 70, 300])
def test_first_valid_beam(gpu, first):
    """transStartInverse comes from the first valid beam (:374-380): in the first wave, the second wave, the
    second chunk."""
    cases = [R.make_case(400, 40 + first, first_valid=first)]
    wants = _check(cases, _run(cases))
    assert not np.any(wants[0]["cloud"][:first]) and np.any(wants[0]["cloud"][first])


def test_no_valid_beam(gpu):
    cases = [R.make_case(300, 50, all_invalid=True), R.make_case(300, 51)]
    got = _run(cases)
    _check(cases, got)
    assert not np.any(got["cloud"][0, :300]) and got["n"][0] == 0 and got["status"][0] == 0


def test_range_edge_values(gpu):
    """NaN, +-inf, below range_min, above range_max, exactly the bounds."""
    c = R.make_case(600, 60)
    r = c["ranges"]
    assert np.isnan(r).any() and np.isposinf(r).any() and np.isneginf(r).any()
    assert (r < np.float32(c["range_min"])).any() and (r[np.isfinite(r)] > np.float32(c["range_max"])).any()
    assert (r == np.float32(c["range_min"])).any() and (r == np.float32(c["range_max"])).any()
    want = _check([c], _run([c]))[0]
    edge = (r == np.float32(c["range_min"])) | (r == np.float32(c["range_max"]))
    assert np.all(want["cloud"][edge, 2] != 0.0)  # the bounds themselves are valid (:351-352 are strict)


@pytest.mark.parametrize("n_imu", [1, 2, 37, 2000])
def test_imu_window_sizes(gpu, n_imu):
    """1 sample cannot cover a sweep (status 1); 2 leave current_imu_index_ = 0; 2000 fills queueLength."""
    cases = [R.make_case(257, 70 + n_imu, n_imu=n_imu)]
    want = _check(cases, _run(cases, max_imu=max(n_imu, 1)))[0]
    assert want["status"] == (1 if n_imu == 1 else 0)


@pytest.mark.parametrize("mode,status", [("hit", 0), ("early_end", 0), ("at_start", 1), ("late", 1), ("short", 1)])
def test_imu_window_shapes(gpu, mode, status):
    """A point time equal to a sample time (the strict < of :408), point times after the last in-window sample
    (the > branch of :414), a sample exactly at the scan start, a late first and an early last sample (:183-184)."""
    cases = [R.make_case(300, 80, n_imu=24, imu_mode=mode)]
    want = _check(cases, _run(cases))[0]
    assert want["status"] == status
    if status:
        assert not np.any(want["cloud"]) and want["n"] == 0


def test_imu_pointer_front_zero(gpu):
    """Only one sample before the scan and one after it: imuPointerFront == 0 for every beam (:414), rotation 0."""
    a = R.make_case(129, 90, n_imu=2)
    b = dict(a, use_imu=False)
    wa = _check([a], _run([a]))[0]
    assert R.bits_equal(wa["cloud"], R.correct(b)["cloud"])


def test_imu_count_outside_window_is_status_1(gpu):
    """A device-side sample count past max_imu is reported, not read."""
    c = R.make_case(64, 95, n_imu=9)
    f = _fleet_for([c], max_imu=8)
    got = _run([c], fleet=f)
    f.close()
    assert got["status"][0] == 1 and got["n"][0] == 0 and not np.any(got["cloud"][0, :64])


@pytest.mark.parametrize("use_imu,use_odom", [(False, True), (True, False), (False, False)])
def test_sources_off(gpu, use_imu, use_odom):
    cases = [R.make_case(300, 110, use_imu=use_imu, use_odom=use_odom)]
    got = _run(cases)
    _check(cases, got)
    if not use_imu and not use_odom:  # the plain polar projection in the frame z = 1
        c = cases[0]
        r = c["ranges"]
        ok = np.isfinite(r) & ~(r < np.float32(c["range_min"])) & ~(r > np.float32(c["range_max"]))
        want = np.zeros((300, 3), np.float32)
        want[ok, 0] = (r[ok].astype(np.float64) * c["cs"][ok, 0]).astype(np.float32)
        want[ok, 1] = (r[ok].astype(np.float64) * c["cs"][ok, 1]).astype(np.float32)
        want[ok, 2] = 1.0
        assert R.bits_equal(got["cloud"][0, :300], want)


def test_equal_odom_times(gpu):
    """start_odom_time_ == end_odom_time_: the ratio of :442 is +-inf, the points are what IEEE gives."""
    cases = [R.make_case(300, 120, odom_mode="equal")]
    want = _check(cases, _run(cases))[0]
    assert not np.isfinite(want["cloud"]).all() and want["status"] == 0


def test_either_output_may_be_null(gpu):
    cases = [R.make_case(257, 130), R.make_case(257, 131, n_imu=3)]
    _check(cases, _run(cases, want_cloud=False))
    _check(cases, _run(cases, want_xy=False))


def test_tilted_rules_and_zero_points(gpu):
    """A pitched, offset laser with a negative lower distance bound: the zero points of invalid beams pass the
    distance test and meet the z window like any other cloud point (hector_slam.cc:331-357)."""
    cases = [R.make_case(300, 140, rules=R.TILTED_RULES, scale=10.0)]
    want = _check(cases, _run(cases))[0]
    assert np.any(want["origo"] != 0.0)


def test_golden_fixture_on_the_device(gpu):
    cases = R.load_golden()
    for name, (c, want) in cases.items():
        _check([c], _run([c]), wants=[want])


def test_default_laser_and_argument_checks(gpu):
    L = default_laser(1081, -1.0, 0.01)
    d = L.as_oracle_dict()
    got = {"tf": d["tf"], "use_max": d["use_max"], "sqr_min": d["sqr_min"], "sqr_max": d["sqr_max"],
           "z_min": d["z_min"], "z_max": d["z_max"]}
    assert got == R.DEFAULT_RULES
    lib = UndistortFleet(1, 8, 4).L
    h = C.c_void_p()
    assert lib.ud_create(C.byref(h), 1, 8, 2001) == -1 and b"2000" in lib.ud_last_error()   # UD_EINVAL
    assert lib.ud_create(C.byref(h), 1, 8, 0) == -1
    f = UndistortFleet(1, 8, 4)
    with pytest.raises(Exception, match="ud_set_scan_geometry"):
        f.correct(np.ones(8, np.float32), 0.0, 0.01, np.zeros((2, 4)), np.zeros((2, 7)))
    f.close()


def test_host_entry_and_node_mirror(gpu):
    """ud_correct (one scan from host memory) equals the batch entry; IMU times that decrease are UD_EINVAL;
    LidarUndistortion.ScanCallback feeds the same record through."""
    c = R.make_case(360, 150, n_imu=24)
    want = R.correct(c)
    f = _fleet_for([c])
    got = f.correct(c["ranges"], c["t_start"], c["t_inc"], c["imu"], c["odom"])
    assert got["status"] == 0 and got["n"] == want["n"]
    assert R.bits_equal(got["cloud"], want["cloud"]) and R.bits_equal(got["xy"], want["xy"])
    assert R.bits_equal(got["origo"], want["origo"])
    bad = c["imu"].copy()
    bad[[5, 6]] = bad[[6, 5]]
    assert bad[6, 0] < bad[5, 0]
    with pytest.raises(Exception, match="non-decreasing"):
        f.correct(c["ranges"], c["t_start"], c["t_inc"], bad, c["odom"])
    f.close()
    # the node: two scans, IMU at 100 Hz, odometry at 50 Hz (identity orientation, moving along x)
    n = 360
    f = UndistortFleet(1, n, 64)
    ainc = float(np.float32(2.0 * np.pi / n))
    cs = R.unit_vectors(n, R.AMIN, ainc)
    f.set_scan_geometry(R.AMIN, ainc, 0.15, 20.0)  # the library's own CreateAngleCache
    node = LidarUndistortion(f)
    for k in range(40):
        node.ImuCallback(99.9 + 0.01 * k, (0.01, -0.02, 0.4))
    for k in range(20):
        node.OdomCallback(99.9 + 0.02 * k, (0.5 * 0.02 * k, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))
    tinc = 0.1 / n
    ranges = np.linspace(1.0, 9.0, n).astype(np.float32)
    assert node.ScanCallback(100.0, tinc, ranges) is None
    rec = node.ScanCallback(100.1, tinc, ranges)
    assert rec["status"] == 0 and rec["n"] > 0
    case = {"n": n, "ranges": ranges, "cs": cs, "range_min": 0.15, "range_max": 20.0, "t_start": rec["scan_time"][0],
            "t_inc": rec["scan_time"][1], "use_imu": True, "use_odom": True, "imu": rec["imu"], "odom": rec["odom"],
            "rules": R.DEFAULT_RULES, "scale": 20.0}
    want = R.correct(case)
    assert R.bits_equal(rec["cloud"], want["cloud"]) and R.bits_equal(rec["xy"], want["xy"])
    f.close()


def test_composition_with_hector_step_device(gpu):
    """2 streams x 3 scans, 512^2 x 2 levels: ud_correct_batch_device's d_xy / d_n / d_origo go straight into
    HectorFleet.step_device; poses and maps equal O.HectorOracle.process fed the restatement's container points."""
    import torch

    S, T, LV, SIZE, N = 2, 3, 2, 512, 1081
    scans = synth.make_streams(S, T, with_points=False, seed=23)
    ang = synth.beam_angles(N)
    cs = np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], 1))
    hf = HectorFleet(S, 0.05, SIZE, (0.5, 0.5), LV, max_points=N)
    hf.set_update_factors(0.4, 0.9)
    hf.set_thresholds(-1.0, -1.0)
    oras = [O.HectorOracle(0.05, SIZE, (0.5, 0.5), LV, reduce_threads=0) for _ in range(S)]
    for o in oras:
        o.set_update_factors(0.4, 0.9)
        o.set_thresholds(-1.0, -1.0)
    scale = hf.scale_to_map()
    rules = dict(R.DEFAULT_RULES)
    rules["tf"] = list(rules["tf"][:9]) + [0.12, -0.05, 0.3]  # a mounted laser: origo != 0
    uf = UndistortFleet(S, N, 32)
    uf.set_scan_geometry(0.0, 0.0, 0.1, 30.0, unit_vectors=cs)
    uf.set_container_rules(_laser(rules), scale)
    rng = np.random.default_rng(5)
    st = torch.cuda.Stream()
    for t in range(T):
        cases = []
        for s in range(S):
            t0 = 50.0 + 0.1 * t
            tinc = float(np.float32(0.1 / N))
            ti = np.concatenate([[t0 - 0.004], np.sort(rng.uniform(t0, t0 + tinc * (N - 1), 20)), [t0 + 0.11]])
            imu = np.concatenate([ti[:, None], rng.uniform(-0.02, 0.02, (22, 2)), rng.uniform(-0.4, 0.4, (22, 1))], 1)
            o0 = np.array([t0 - 0.01, 1.0 + s, 2.0, 0.0, 0.0, 0.0, 0.3 * s])
            o1 = o0 + np.array([0.09, 0.03, -0.02, 0.0, 0.0, 0.0, 0.01])
            cases.append({"n": N, "ranges": np.ascontiguousarray(scans.ranges[s, t]), "cs": cs, "range_min": 0.1,
                          "range_max": 30.0, "t_start": t0, "t_inc": tinc, "use_imu": True, "use_odom": True,
                          "imu": imu, "odom": np.stack([o0, o1]), "rules": rules, "scale": scale})
        d_r = torch.from_numpy(np.stack([c["ranges"] for c in cases])).cuda()
        d_tm = torch.from_numpy(np.array([[c["t_start"], c["t_inc"]] for c in cases])).cuda()
        d_imu = torch.from_numpy(np.stack([c["imu"] for c in cases])).cuda()
        d_in = torch.full((S,), 22, dtype=torch.int32, device="cuda")
        d_od = torch.from_numpy(np.stack([c["odom"] for c in cases])).cuda()
        d_xy = torch.zeros((S, N, 2), dtype=torch.float32, device="cuda")
        d_n = torch.zeros((S,), dtype=torch.int32, device="cuda")
        d_o = torch.zeros((S, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        # both calls on one HIP stream: the Hector step is ordered after the undistortion by the stream itself
        uf.correct_device(S, d_r, N, d_tm, d_imu, 22, d_in, d_od, None, 0, d_xy, N, d_n, d_o, None,
                          hip_stream=st.cuda_stream)
        hf.step_device(d_xy.data_ptr(), N, d_n.data_ptr(), d_o.data_ptr(), hip_stream=st.cuda_stream)
        st.synchronize()
        gp, _, gd, _ = hf.poses()
        for s in range(S):
            w = R.correct(cases[s])
            assert w["status"] == 0 and w["n"] > 500
            op, _, od = oras[s].process(w["xy"], origo=tuple(w["origo"]))
            assert gd[s] == od, (t, s)
            assert np.array_equal(gp[s].view(np.int32), op.view(np.int32)), (t, s, gp[s], op)
    for s in range(S):
        for lvl in range(LV):
            m = hf.get_map(s, lvl)
            ol, ou = oras[s].level(lvl)
            assert np.array_equal(m["upd"], ou)
            assert np.array_equal(m["logodds"].view(np.int32), ol.view(np.int32))
    uf.close()
    hf.close()
