"""The Karto scan-intake stage without a GPU (include/slam2d/karto_process.h): the CPU restatement
tests/ref/karto_process_ref.c equals the literal transcription tests/ref/karto_process_plain.py and the golden fixture
byte for byte (but for the sign and payload of NaNs, karto_process_ref.canonical_nans) on the directed cases of the
gate, the carry, the trim and the refusals; the host code of kp_create / kp_set_state / kp_commit_vertices runs in a
stand-alone program under ASan + UBSan; the public interface is exported and refuses what it must without a device."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "ref"))
import karto_process_cases as K  # noqa: E402
import karto_process_plain as P  # noqa: E402
import karto_process_ref as R  # noqa: E402
import make_karto_process_golden as G  # noqa: E402

from slam2d import karto_link as ke  # noqa: E402
from slam2d import karto_loop as kl  # noqa: E402
from slam2d import karto_process as kp  # noqa: E402


@pytest.fixture(scope="module")
def restated():
    """Every directed round through the restatement, computed once."""
    return G.rounds(R)


@pytest.fixture(scope="module")
def plain():
    """The same through the transcription."""
    return G.rounds(P)


@pytest.fixture(scope="module")
def golden():
    return G.load()


# ------------------------------------------------------------------------------------ 1. restatement == plain == golden
@pytest.mark.parametrize("name", list(K.directed_worlds()) + ["moved_1", "moved_2"])
def test_restatement_equals_plain_and_golden(restated, plain, golden, name):
    K.assert_same_step(restated[name], golden[name], f"{name} against the golden")
    K.assert_same_step(restated[name], plain[name], f"{name} against the transcription")


def test_fleets_equal_plain():
    for n_graphs, nr, inverted in ((1, 8, 0), (5, 67, 1), (40, 8, 0), (40, 3, 1)):
        for seed in range(3):
            w = K.fleet_world(n_graphs, nr, seed, inverted)
            K.assert_same_step(K.step(R, w), K.step(P, w), f"fleet of {n_graphs}, seed {seed}")


# ------------------------------------------------------------------------------------ 2. the cases have their properties
def test_gate_cases_by_hand(restated):
    rec = restated["gate"]["rec"]
    assert rec["accepted"].tolist() == [int(a) for a in K.gate_expected()]
    assert not rec["status"].any()
    names = list(K.GATE)
    # the exact thresholds are met exactly: the squared distances and the heading differences are the thresholds' bits
    for name, thr in (("distance_at_threshold", K.THR_TRAVEL), ("distance_one_ulp_below", K.up(K.THR_TRAVEL, -1))):
        x, y, _ = K.GATE[name][2]
        assert x * x + y * y == thr
    assert K.THR_TRAVEL == R.threshold(0.2) and K.THR_BUFFER == R.threshold(20.0)
    assert R.sensor_at(K.GATE["heading_at_threshold"][2])[2] == K.HEADING
    wrapped = R.sensor_at(K.GATE["heading_wraps"][2])[2]
    assert abs(wrapped + 0.1) < 1e-12  # 2 pi - 0.1 is -0.1 after NormalizeAngle
    # a rejected candidate has its poses, no scan, and writes nothing but its record
    r = rec[names.index("nothing")]
    assert (r["scan"], r["job"], r["seq"], r["prev"]) == (-1, -1, -1, 0) and r["corrected"].tolist() == [0.05, 0.05, 0.05]
    first = rec[len(names)]
    assert (first["scan"], first["prev"], first["seq"], first["accepted"]) == (0, -1, -1, 1)
    assert first["corrected"].tolist() == [1.5, -2.0, 0.7]  # corrected = odom (karto_slam.cc:439-440)
    o = restated["gate"]["intake"]
    n_acc = int(rec["accepted"].sum())
    assert int(o["n_jobs"][0]) == n_acc and int(o["n_seq"][0]) == n_acc - 1
    assert rec["job"][rec["accepted"] == 1].tolist() == list(range(n_acc))
    w = K.case_gate()
    untouched = np.ones(len(w["pool_poses"]), bool)
    for g in np.flatnonzero(rec["accepted"]):
        untouched[int(w["pool_offset"][g]) + int(rec["scan"][g])] = False
    R.assert_same_records(o["pool_poses"][untouched], w["pool_poses"][untouched], "pool rows of rejected candidates")
    R.assert_same_records(o["pool_ranges"][untouched], w["pool_ranges"][untouched], "range rows of rejected candidates")
    # the records after the counts keep their poison
    assert o["jobs"][n_acc:].tobytes() == R.poisoned(len(rec) - n_acc, R.JOB).tobytes()


def test_carry_cases_by_hand(restated):
    s = restated["carry"]
    rec0 = s["intake"]["rec"]
    assert rec0["accepted"].all()
    # graph 0: the identity branch -- the corrected pose is the odometric pose with its heading normalised
    assert rec0[0]["corrected"].tolist() == [1.3, 2.2, 0.6]
    # graph 1: the last odometric pose at the origin position: transform position = the last corrected pose's
    import karto_link_ref as LR
    dh = 0.5 - 0.3
    x = 1.0 + (LR.cos(dh) * 0.4 + (0.0 - LR.sin(dh)) * -0.1 + 0.0 * 0.45)
    assert rec0[1]["corrected"][0] == x and rec0[1]["corrected"][2] == 0.45 + (0.5 - 0.3)
    # graph 4: a first scan keeps its odometric heading as given; its sensor pose has it normalised
    assert rec0[4]["corrected"][2] == 7.0 and rec0[4]["sensor"][2] == 7.0 - 2.0 * math.pi
    assert np.isnan(rec0[5]["corrected"][0]) and rec0[5]["accepted"] == 1
    # apply: the matched pose to the pool, but for the KT_ERANGE match, which leaves the predicted pose
    rec = s["rec"]
    assert rec["match_status"].tolist() == [0, 0, R.KT_ERANGE, 0, 0, 0]
    assert rec[0]["sensor"].tolist() == [1.31, 2.19, 0.61] and rec[0]["corrected"].tolist() == [1.31, 2.19, 0.61]
    R.assert_same_records(rec[2], _with(rec0[2], match_status=R.KT_ERANGE), "the KT_ERANGE match")
    assert rec[5]["sensor"].tolist() == [1.0, 1.0, 9.0] and rec[5]["corrected"][2] == LR.normalize_angle(9.0)
    R.assert_same_records(rec[4], rec0[4], "a first scan is not matched")


def _with(r, **kw):
    r = np.array(r, copy=True)
    for k, v in kw.items():
        r[k] = v
    return r


def test_moved_pose_is_read_at_the_next_intake(restated):
    a, b = restated["moved_1"], restated["moved_2"]
    assert a["rec"]["accepted"].tolist() == [1] and b["rec"]["accepted"].tolist() == [1]
    assert a["adv"][0]["corrected"].tolist() == [1.08, 0.27, 0.24]  # GetCorrectedPose() at the final pose
    w, edit, cands = K.moved_sequence()
    unmoved = K.step(R, K.next_world(w, K.step(R, w), cands))
    assert b["rec"][0]["corrected"].tolist() != unmoved["rec"][0]["corrected"].tolist()
    assert b["states"][0]["n_scans"] == 4 and b["intake"]["base_index"][:3].tolist() == [0, 1, 2]


def test_trim_cases_by_hand(restated):
    for name, (w, want) in K.trim_cases().items():
        s = restated[f"trim_{name}"]
        a = s["adv"][0]
        assert (int(a["run_begin"]), int(a["run_length"])) == want, name
        st = s["states"][0]
        n = int(w["states"][0]["n_scans"])
        assert (st["n_scans"], st["run_begin"], st["run_length"]) == (n + 1, want[0], want[1]) and a["n_scans"] == n + 1
        assert st["last_time"] == 4000.0 and st["last_odom"].tolist() == w["cand"][0]["odom"].tolist()
    for name, thr in (("d2_at_threshold", K.THR_BUFFER), ("d2_one_ulp_above", K.up(K.THR_BUFFER, 1))):
        x, y, _ = K.trim_cases()[name][0]["pool_poses"][0]
        assert x * x + y * y == thr
    assert K.trim_cases()["69_of_70"][0]["states"][0]["run_length"] == 70  # more than one round of 64 fronts


def test_refusal_cases_by_hand(restated):
    rec = restated["refusals"]["rec"]
    assert rec["status"].tolist() == [R.KP_ERANGE, 0, R.KP_EINVAL, 0, R.KP_EINVAL] and not rec["accepted"].any()
    assert rec["prev"].tolist() == [3, 3, 0, -1, -1]
    o = restated["refusals"]["intake"]
    w = K.case_refusals()
    assert int(o["n_jobs"][0]) == 0 and int(o["n_seq"][0]) == 0 and o["base_begin"][0] == 0
    R.assert_same_records(o["pool_poses"], w["pool_poses"], "nothing is written")
    R.assert_same_records(restated["refusals"]["states"], w["states"], "no state moves")
    rec = restated["refusals_tail"]["rec"]
    assert rec["status"].tolist() == [0, 0, 0, R.KP_EINVAL, R.KP_EINVAL] and rec["accepted"].tolist() == [1, 1, 1, 0, 0]
    for args in K.refused_creates():
        assert not R.check_create(*args), args
    for args in K.accepted_creates():
        assert R.check_create(*args), args


def test_inverted_rows_are_reversed(restated):
    w = K.directed_worlds()["inverted"]
    s = restated["inverted"]
    acc = np.flatnonzero(s["rec"]["accepted"])
    assert len(acc) >= 2
    for i in acc:
        slot = int(w["pool_offset"][i]) + int(s["rec"]["scan"][i])
        want = w["ranges_f32"][int(w["cand"][i]["row"])][::-1].astype(np.float64)
        R.assert_same_records(s["intake"]["pool_ranges"][slot], want, f"graph {i}")


def test_bind_near_equals_plain():
    rng = np.random.default_rng(12)
    for n_jobs in (1, 3, 9):
        for _ in range(5):
            slots = np.sort(rng.integers(0, n_jobs, int(rng.integers(0, 12))))
            src = np.zeros(len(slots), R.SOURCE)
            src["slot"], src["chain"] = slots, rng.integers(0, 4, len(slots))
            jobs = np.zeros(n_jobs, R.JOB)
            a, b = R.bind_near(jobs, n_jobs, src, len(src)), P.bind_near(jobs, n_jobs, src, len(src))
            R.assert_same_records(a, b, "near ranges")
            assert int(a["near_count"].sum()) == len(src)


# ------------------------------------------------------------------------------------ 3. the host code, stand-alone
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tests/cpp/karto_process_check.cpp under ASan + UBSan; a stand-alone program."""
    exe = str(tmp_path_factory.mktemp("kp_check") / "karto_process_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan",
                    "-static-libubsan", "-fno-sanitize-recover=all", "-I", R.CSRC,
                    os.path.join(HERE, "cpp", "karto_process_check.cpp"), "-o", exe], check=True)

    def run(*words):
        r = subprocess.run([exe], input=" ".join(str(v) for v in words) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        return json.loads(r.stdout)

    return run


def test_host_create_rules(host_check):
    def create(p, nr, ms, n_graphs=3):
        return host_check("create", *[p[k] for k in R.PARAM_FIELDS], n_graphs, nr, ms)

    for args in K.refused_creates():
        out = create(*args)
        assert out["ok"] == 0 and out["why"], args
    for args in K.accepted_creates():
        out = create(*args)
        assert out["ok"] == 1, (args, out)
        assert float.fromhex(out["thr_travel"]) == R.threshold(args[0]["minimum_travel_distance"])
        assert float.fromhex(out["thr_buffer"]) == R.threshold(args[0]["scan_buffer_maximum_scan_distance"])
        assert out["window_max"] == min(args[0]["scan_buffer_size"], args[2])
    assert create(R.DEFAULT_PARAMS, 8, 16, n_graphs=0)["ok"] == 0
    assert create(dict(R.DEFAULT_PARAMS, inverted=2), 8, 16)["ok"] == 0


def test_host_state_rule(host_check):
    ok = [(0, 0, 0), (1, 0, 1), (5, 2, 3), (5, 4, 1), (16, 13, 3)]
    bad = [(0, 0, 1), (0, 1, 0), (5, 2, 2), (5, 0, 5), (5, 5, 0), (3, 0, 0), (17, 14, 3), (-1, 0, 0), (5, 3, 3), (4, -1, 5)]
    for n, b, l_ in ok:
        assert host_check("state", n, b, l_, 16, 3)["ok"] == 1, (n, b, l_)
    for n, b, l_ in bad:
        assert host_check("state", n, b, l_, 16, 3)["ok"] == 0, (n, b, l_)


def test_host_vertex_plan(host_check):
    # graphs 1 .. 4 of 5; records: accepted, rejected, refused (never a vertex), accepted
    out = host_check("commit", 5, 1, 4, -1, 9, 2, 0, 7, 3, 0, 1, 2, 0, 0, -1, R.KP_ERANGE, 0, -1, 0, 1, 3)
    assert out == dict(added=2, ok=1, mismatch=0, vertices=[[1, 2], [4, 3]], nodes=[[1, 2, 102.0], [4, 3, 403.0]],
                       counts=[9, 3, 0, 7, 4])
    # a scan index that is not the graph's scan count: the vertex is added, no node, the plan ends
    out = host_check("commit", 2, 0, 2, -1, 2, 5, 0, 1, 3, 0, 1, 5)
    assert (out["ok"], out["mismatch"], out["added"], out["nodes"], out["counts"]) == (0, 1, 1, [], [3, 5])
    # AddNode's refusal ends the plan; what went before stays
    out = host_check("commit", 3, 0, 3, 1, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0)
    assert (out["ok"], out["mismatch"], out["added"]) == (0, 0, 2) and out["nodes"] == [[0, 0, 0.0]] and out["counts"] == [1, 1, 0]
    # a record with accepted set and a status is not committed
    out = host_check("commit", 1, 0, 1, -1, 0, R.KP_EINVAL, 1, 0)
    assert (out["ok"], out["added"], out["counts"]) == (1, 0, [0])


# ------------------------------------------------------------------------------------ 4. the public interface
def test_abi_is_exported_and_layouts_match():
    hdr = open(os.path.join(REPO, "include", "slam2d", "karto_process.h")).read()
    names = sorted(set(re.findall(r"\b(kp_[a-z_]+)\s*\(", hdr)))
    assert {"kp_create", "kp_destroy", "kp_intake_device", "kp_apply_match_device", "kp_commit_vertices",
            "kp_bind_near_device", "kp_advance_device", "kp_get_intake", "kp_get_state", "kp_set_state", "kp_clear_graph",
            "kp_result_device", "kp_last_error", "kp_version", "kp_default_params", "kp_node_params", "kp_set_timing",
            "kp_num_kernels", "kp_kernel_name", "kp_get_kernel_times"} == set(names)
    L = kp._lib.lib()
    kp._declare(L)
    for n in names:
        assert hasattr(L, n), f"{n} is declared in karto_process.h but not exported by libslam2d.so"
    assert ctypes.sizeof(kp.KpParams) == 40 == ctypes.sizeof(R.Params)
    assert ctypes.sizeof(kp.KpCandidate) == 40 == R.CANDIDATE.itemsize and R.CANDIDATE == kp.CANDIDATE_DTYPE
    assert ctypes.sizeof(kp.KpIntake) == 88 == R.INTAKE.itemsize and R.INTAKE == kp.INTAKE_DTYPE
    assert ctypes.sizeof(kp.KpAdvanced) == 40 == R.ADVANCED.itemsize and R.ADVANCED == kp.ADVANCED_DTYPE
    assert ctypes.sizeof(kp.KpState) == 48 == R.STATE.itemsize and R.STATE == kp.STATE_DTYPE
    assert R.JOB == ke.JOB_DTYPE and R.SOURCE == kl.SOURCE_DTYPE and R.QUERY.itemsize == 20 and R.ITEM.itemsize == 16
    assert [k for k, _ in kp.KpParams._fields_] == list(R.PARAM_FIELDS)
    assert "#define KP_ERANGE (-5)" in hdr and "#define KP_EINVAL (-1)" in hdr
    assert (R.KP_EINVAL, R.KP_ERANGE) == (kp.KP_EINVAL, kp.KP_ERANGE)
    assert L.kp_version().decode().startswith("slam2d-karto-process")
    kn = [L.kp_kernel_name(i).decode() for i in range(L.kp_num_kernels())]
    assert kn == ["kp_intake_kernel", "kp_compact_kernel", "kp_store_kernel", "kp_apply_kernel", "kp_bind_near_kernel",
                  "kp_advance_kernel"]
    assert L.kp_kernel_name(-1) == b"" and L.kp_kernel_name(len(kn)) == b""
    import slam2d
    assert slam2d.ProcessStage is kp.ProcessStage


def test_params():
    d, n = kp.default_params(), kp.node_params()
    assert [getattr(d, k) for k in R.PARAM_FIELDS] == [R.DEFAULT_PARAMS[k] for k in R.PARAM_FIELDS]
    assert [getattr(n, k) for k in R.PARAM_FIELDS] == [R.NODE_PARAMS[k] for k in R.PARAM_FIELDS]
    assert d.minimum_travel_heading == 10.0 * (math.pi / 180.0) or abs(d.minimum_travel_heading - math.radians(10)) < 1e-15
    assert kp.default_params(scan_buffer_size=5).scan_buffer_size == 5
    with pytest.raises(TypeError):
        kp.default_params(no_such_parameter=1)


def test_argument_refusals_need_no_device():
    L = kp._lib.lib()
    kp._declare(L)
    h = ctypes.c_void_p()
    assert L.kp_create(None, None, 1, 8, 16, None) == kp.KP_EINVAL and "out is NULL" in L.kp_last_error().decode()
    for params, nr, ms in K.refused_creates():
        p = kp.default_params(**params)
        assert L.kp_create(ctypes.byref(h), ctypes.byref(p), 2, nr, ms, None) == kp.KP_EINVAL, (params, nr, ms)
        assert not h.value and L.kp_last_error()
    p = kp.default_params()
    assert L.kp_create(ctypes.byref(h), ctypes.byref(p), 0, 8, 16, None) == kp.KP_EINVAL
    off = (ctypes.c_int * 2)(0, -1)
    assert L.kp_create(ctypes.byref(h), ctypes.byref(p), 2, 8, 16, off) == kp.KP_EINVAL and "offset" in L.kp_last_error().decode()
    # a NULL context is refused by every entry point, and destroying one is a no-op
    z = ctypes.c_int(0)
    assert L.kp_destroy(None) == 0
    assert L.kp_intake_device(None, 0, 0, None, None, 0, None, None, 1, None, None, None, 0, *([None] * 6)) == kp.KP_EINVAL
    assert L.kp_apply_match_device(None, None, 0, None, 1, None) == kp.KP_EINVAL
    assert L.kp_commit_vertices(None, None, None, ctypes.byref(z)) == kp.KP_EINVAL
    assert L.kp_bind_near_device(None, None, None, None, 0, None) == kp.KP_EINVAL
    assert L.kp_advance_device(None, None, 1, None) == kp.KP_EINVAL
    assert L.kp_get_intake(None, 0, 0, None, None) == kp.KP_EINVAL and L.kp_get_state(None, 0, None) == kp.KP_EINVAL
    assert L.kp_set_state(None, 0, None) == kp.KP_EINVAL and L.kp_clear_graph(None, 0) == kp.KP_EINVAL
    assert L.kp_result_device(None, None, None, None, None) == kp.KP_EINVAL and L.kp_set_timing(None, 1) == kp.KP_EINVAL
    assert L.kp_get_kernel_times(None, None, None, 0) == kp.KP_EINVAL
