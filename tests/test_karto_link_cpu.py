"""The Karto graph-linking stage without a GPU: the C restatement the GPU is held to (tests/ref/karto_link_ref.c)
against the literal transcription of the reference members (tests/ref/karto_link_plain.py) and the golden fixture,
byte for byte; hand-derived results of the directed cases; csrc/karto_link_commit.h through a stand-alone C++ program
under ASan + UBSan; the ABI of include/slam2d/karto_link.h in libslam2d.so and the argument refusals that need no
device."""
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
import karto_link_cases as K  # noqa: E402
import karto_link_plain as P  # noqa: E402
import karto_link_ref as R  # noqa: E402
import make_karto_link_golden as G  # noqa: E402

from slam2d import karto as kt  # noqa: E402
from slam2d import karto_link as ke  # noqa: E402
from slam2d import karto_loop as kl  # noqa: E402

SWEEP_WORLDS = 3000   # about 9000 jobs
SWEEP_LOOPS = 1500


def same_stage1(got, want, what):
    for g, w, k in zip(got, want, ("links", "out", "pool")):
        R.assert_same_records(g, w, f"{what} {k}")


def loop_pass(lw, seed=1):
    """The restatement's coarse and fine calls on a loop world with its synthetic fine matches."""
    co = R.loop_coarse(lw)
    fine = K.fine_results(np.random.default_rng(seed), lw, co["fine_of"], co["n_fine"])
    closures, _ = R.loop_fine(lw, co["fine_of"], co["n_fine"], fine)
    return co, fine, closures


# ------------------------------------------------------------------------------------ 1. restatement == transcription
@pytest.mark.parametrize("name", list(K.stage1_cases()))
def test_restatement_equals_plain_on_directed_worlds(name):
    w = K.stage1_cases()[name]
    same_stage1(R.add_edges(w), P.add_edges(w), name)


@pytest.mark.parametrize("name", list(K.loop_cases()))
def test_loop_restatement_equals_plain_on_directed_worlds(name):
    lw = K.loop_cases()[name]
    co, fine, closures = loop_pass(lw)
    want_of, want_closing = G.plain_loop(lw)
    # the transcription knows no capacity: the kept matches are the first of its list
    assert co["info"][0] == len(want_of)
    np.testing.assert_array_equal(co["fine_of"][:co["n_fine"]], want_of[:co["n_fine"]])
    kept = set(co["fine_of"][:co["n_fine"]].tolist())
    m0 = 0
    for s in range(lw["count"]):
        n = int(np.sum(lw["source"]["slot"] == s))
        chains = [(lw["coarse"][m0 + k], {"response": lw["fine_response"][m0 + k]}) for k in range(n)]
        # chains cut off by the capacity never reach the fine match: the transcription sees them coarse-rejected
        chains = [(c if m0 + k in kept else dict(response=-1.0, covariance=c["covariance"]), f)
                  for k, (c, f) in enumerate(chains)]
        assert closures[s]["chain"] == P.try_close_loop(lw["params"], chains)[1], (name, s)
        m0 += n
    if co["n_fine"] == len(want_of):
        np.testing.assert_array_equal(closures["chain"], want_closing)


def test_link_info_and_weighted_mean_equal_plain_bit_for_bit():
    rng = np.random.default_rng(3)
    for k in range(400):
        p1, p2 = rng.uniform(-30, 30, 3), rng.uniform(-30, 30, 3)
        if k % 7 == 0:
            p1[:2] = 0.0
        if k % 21 == 0:
            p1[2] = 0.0
        cov = K.spd(rng)
        st, diff, prec = R.link_info(p1, p2, cov)
        li = P.LinkInfo(P.Pose2(*p1), P.Pose2(*p2), P.Matrix3(cov))
        assert st == R.KE_OK
        np.testing.assert_array_equal(R.bits(diff), R.bits(li.pose_difference.tolist()))
        np.testing.assert_array_equal(R.bits(prec), R.bits(P.precision_matrix(li).tolist()))
        assert -math.pi <= diff[2] <= math.pi
        n = 1 + k % 5
        means, covs = rng.uniform(-8, 8, (n, 3)), np.array([K.spd(rng) for _ in range(n)])
        st, pose = R.weighted_mean(means, covs)
        want = P.compute_weighted_mean([P.Pose2(*m) for m in means], [P.Matrix3(c) for c in covs])
        assert st == R.KE_OK
        np.testing.assert_array_equal(R.bits(pose), R.bits(want.tolist()))


def test_normalize_angle_as_written():
    for a in (0.0, 3.0, -3.0, math.pi, -math.pi, 3.2, -3.2, 6.3, -6.3, 7.5, -13.2, 1e3, -1e3, 4.0e9, -4.0e9):
        got = R.normalize_angle(a)
        assert R.bits(got) == R.bits(P.normalize_angle(a)) and -math.pi <= got <= math.pi, a
    # the cast branch is taken literally: one multiple of 2 pi, not fmod
    assert R.normalize_angle(20.0) == 20.0 - 3 * 6.28318530717958647692
    for a in (math.inf, -math.inf, math.nan, 4294967296.0, -1e300):
        assert math.isnan(R.normalize_angle(a)) and math.isnan(P.normalize_angle(a))


def test_random_sweep_equals_plain_and_exercises_every_exit():
    """A few thousand jobs in worlds of 1 .. 5 and as many loop worlds: byte-identical to the transcription, and every
    exit of the directed list is met at least once."""
    met, jobs = set(), 0
    for seed in range(SWEEP_WORLDS):
        w = K.random_world(seed)
        got = R.add_edges(w)
        same_stage1(got, P.add_edges(w), f"seed {seed}")
        met |= K.stage1_exits(w, got[0], got[1])
        jobs += len(w["jobs"])
    lmet = set()
    for seed in range(SWEEP_LOOPS):
        lw = K.random_loop_world(seed)
        co, fine, closures = loop_pass(lw, seed)
        want_of, want_closing = G.plain_loop(lw)
        assert co["info"][0] == len(want_of), seed
        np.testing.assert_array_equal(co["fine_of"][:co["n_fine"]], want_of[:co["n_fine"]], err_msg=f"seed {seed}")
        if co["n_fine"] == len(want_of):
            np.testing.assert_array_equal(closures["chain"], want_closing, err_msg=f"seed {seed}")
        lmet |= K.loop_exits(lw, co, closures)
    print(jobs, sorted(met), sorted(lmet))
    assert jobs >= 3000
    assert met == K.STAGE1_EXITS, K.STAGE1_EXITS - met
    assert lmet == K.LOOP_EXITS, K.LOOP_EXITS - lmet


def test_golden_fixture_reproduces():
    stage1, loops = G.load()
    fresh1, freshl = K.stage1_cases(), K.loop_cases()
    assert set(stage1) == set(fresh1) and set(loops) == set(freshl)
    for name, (w, want_links, want_out, want_pool) in stage1.items():
        for k in G.WORLD_KEYS:
            R.assert_same_records(w[k], np.ascontiguousarray(fresh1[name][k]), f"{name} {k}")
        assert w["params"] == fresh1[name]["params"] and w["max_links"] == fresh1[name]["max_links"]
        same_stage1(R.add_edges(w), (want_links, want_out, want_pool), name)
    for name, (lw, want_of, want_closing) in loops.items():
        for k in G.LOOP_KEYS:
            R.assert_same_records(lw[k], np.ascontiguousarray(freshl[name][k]), f"{name} {k}")
        co, fine, closures = loop_pass(lw)
        np.testing.assert_array_equal(co["fine_of"][:co["n_fine"]], want_of[:co["n_fine"]], err_msg=name)
        if co["n_fine"] == len(want_of):
            np.testing.assert_array_equal(closures["chain"], want_closing, err_msg=name)


# ------------------------------------------------------------------------------------ 2. hand-derived results
def test_one_minus_c_case_has_the_property():
    h = K.find_one_minus_c_heading()
    c = R.cos(-h)
    assert (1.0 - c) + c != 1.0
    # FromAxisAngle's [2][2] = 1 * 1 * (1 - c) + c enters the rotated covariance's [2][2]: with a diagonal
    # covariance that entry is m22 * cov22 * m22, not cov22
    st, diff, prec = R.link_info([0.4, -0.3, h], [1.0, 1.0, 0.2], np.diag([1.0, 1.0, 3.0]).reshape(9))
    m22 = (1.0 - c) + c
    assert st == R.KE_OK and m22 * 3.0 * m22 != 3.0
    w = K.case_one_minus_c()
    links, out, _ = R.add_edges(w)
    assert "one_minus_c" in K.stage1_exits(w, links, out)


def test_set_transform_branches_by_hand():
    cov = np.diag([0.01, 0.02, 0.03]).reshape(9)
    # pose1 == Pose2(): identity rotation, so diff is pose2 with its heading normalised
    st, diff, _ = R.link_info([0.0, 0.0, 0.0], [1.25, -2.5, 7.0], cov)
    assert st == 0 and diff[0] == 1.25 and diff[1] == -2.5 and diff[2] == 7.0 - 6.28318530717958647692
    st, diff2, _ = R.link_info([-0.0, 0.0, -0.0], [1.25, -2.5, 7.0], cov)
    np.testing.assert_array_equal(R.bits(diff2), R.bits(diff))
    # pose1 at the origin position, heading pi / 2: a pure rotation by -pi / 2 (through detmath's sin / cos)
    st, diff, _ = R.link_info([0.0, 0.0, math.pi / 2], [1.0, 0.0, math.pi / 2], cov)
    assert st == 0 and abs(diff[0]) < 1e-15 and abs(diff[1] + 1.0) < 1e-15 and diff[2] == 0.0
    # the general case: pose2 == pose1 gives a zero difference up to rounding
    st, diff, _ = R.link_info([3.0, -4.0, 0.5], [3.0, -4.0, 0.5], cov)
    assert st == 0 and np.all(np.abs(diff) < 1e-15)


def test_threshold_and_status_cases_by_hand():
    w = K.case_threshold()
    links, out, _ = R.add_edges(w)
    thr = K.threshold(w["params"])
    assert w["near"]["response"][0] == thr and w["near"]["response"][1] == np.nextafter(thr, math.inf)
    # prev + running + the matches one ulp above and at link_min; the one at the threshold, below it and NaN are out
    assert (out[0]["n_links"], out[0]["n_means"], out[0]["status"]) == (4, 3, 0)
    assert links[0]["kind"][:4].tolist() == [R.KE_PREV, R.KE_RUNNING, R.KE_NEAR, R.KE_NEAR]
    w = K.case_singular()
    links, out, pool = R.add_edges(w)
    assert out["status"].tolist() == [R.KE_SINGULAR] * 4 + [0, 0]
    assert links[0]["status"][:5].tolist() == [0, 0, 0, R.KE_SINGULAR, 0]      # the other records are still emitted
    assert not links[0]["diff"][3].any() and not links[0]["precision"][3].any()  # and no garbage in the refused one
    assert links[1]["status"][:4].tolist() == [0, 0, R.KE_SINGULAR, 0]         # the NaN covariance
    assert links[2]["status"][:3].tolist() == [R.KE_SINGULAR, R.KE_SINGULAR, 0]  # rCovariance singular
    assert links[3]["status"][:3].tolist() == [0, 0, 0]                        # only the sum of inverses is singular
    for j in range(4):
        np.testing.assert_array_equal(R.bits(out[j]["pose"]), R.bits(w["pool_poses"][w["jobs"][j]["pool_offset"] + 4]))
    w = K.case_link_counts()
    links, out, _ = R.add_edges(w)
    assert out["n_links"].tolist() == [0, 1, 2, 63, 64, 0, 3, 64, 2]
    assert out["status"].tolist() == [0, 0, 0, 0, 0, R.KE_ERANGE, 0, 0, 0]
    assert links[5].tobytes() == R.poisoned(64, R.LINK).tobytes()  # the refused job wrote nothing
    assert out[8]["n_means"] == 101 and links[7]["kind"][:64].tolist() == [R.KE_NEAR] * 64
    w = K.case_write_pose()
    links, out, pool = R.add_edges(w)
    S = len(w["pool_poses"]) // 4
    changed = [bool((R.bits(pool[j * S:(j + 1) * S]) != R.bits(w["pool_poses"][j * S:(j + 1) * S])).any()) for j in range(4)]
    assert changed == [True, False, False, False] and out["status"].tolist() == [0, R.KE_SINGULAR, 0, R.KE_ERANGE]
    np.testing.assert_array_equal(R.bits(pool[w["jobs"][0]["scan"]]), R.bits(out[0]["pose"]))
    w = K.case_bad_indices()
    links, out, pool = R.add_edges(w)
    assert out["status"].tolist() == [0] + [R.KE_EINVAL] * 11 and not out["n_links"][1:].any()
    assert links[1:].tobytes() == R.poisoned((11, 64), R.LINK).tobytes()


def test_loop_cases_by_hand():
    cases = K.loop_cases()
    co, fine, cl = loop_pass(cases["coarse_edges"])
    # variance equal to the maximum on either axis, the response at its minimum and NaNs are rejected; only the chain
    # just inside every bound and the second slot's chain go on
    assert co["fine_of"][:co["n_fine"]].tolist() == [5, 6] and co["info"] == (2, 0)
    assert cl["chain"].tolist() == [5, 0, -1, -1] and cl["resume"][1] == cases["coarse_edges"]["loop_chains"][1, 0]["resume"]
    lw = cases["fine_edges"]
    co, fine, cl = loop_pass(lw)
    # slot 0: a NaN fine response is accepted; slot 1: just below the minimum is rejected, the minimum itself accepted;
    # slot 2: both fine matches rejected; slot 3: coarse-rejected, fine-rejected, then the third chain closes
    assert cl["chain"].tolist() == [0, 1, -1, 2] and math.isnan(fine[0]["response"])
    assert cl["fine"].tolist() == [0, 3, -1, 8]
    np.testing.assert_array_equal(R.bits(cl["pose"][3]), R.bits(fine[8]["mean"]))
    m = co["fine_of"][8]
    assert co["fine_base_begin"][9] - co["fine_base_begin"][8] == 7 == lw["base_begin"][m + 1] - lw["base_begin"][m]
    lw = cases["overflow"]
    co, fine, cl = loop_pass(lw)
    assert co["n_fine"] == 7 and co["info"] == (12, R.KE_LOOP_OVERFLOW) and co["fine_of"].tolist() == list(range(7))
    assert co["fine_query"].tolist() == [lw["tmp_first"] + f for f in range(7)]
    for f in range(7):
        np.testing.assert_array_equal(co["tmp_ranges"][f], lw["pool_ranges"][lw["query"][f]])
        np.testing.assert_array_equal(co["tmp_poses"][f], lw["coarse"][f]["mean"])
    lw = cases["base_overflow"]
    co, fine, cl = loop_pass(lw)
    assert co["n_fine"] == 4 and co["info"] == (12, R.KE_LOOP_OVERFLOW) and co["fine_base_begin"][4] <= 11
    assert np.isinf(co["tmp_ranges"][4:]).all() and not co["tmp_poses"][4:].any()
    co, fine, cl = loop_pass(cases["zero_capacity"])
    assert co["n_fine"] == 0 and co["fine_base_begin"].tolist() == [0] and cl["chain"].tolist() == [-1, -1, -1]


# ------------------------------------------------------------------------------------ 3. the host commit
@pytest.fixture(scope="module")
def commit_check(tmp_path_factory):
    """tests/cpp/karto_link_commit_check.cpp under ASan + UBSan; a stand-alone program."""
    exe = str(tmp_path_factory.mktemp("ke_commit") / "karto_link_commit_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan",
                    "-static-libubsan", "-fno-sanitize-recover=all", "-I", R.CSRC,
                    os.path.join(HERE, "cpp", "karto_link_commit_check.cpp"), "-o", exe], check=True)

    def run(n_graphs, n_vertices, max_links, jobs):
        """jobs: [(status, graph, n_links, [(from, to, status), ...])]; unwritten records are padded with garbage."""
        words = [n_graphs, n_vertices, len(jobs), max_links]
        for st, g, n, recs in jobs:
            words += [st, g, n]
            for r in range(max_links):
                words += list(recs[r]) if r < len(recs) else [-99, -99, 0]
        r = subprocess.run([exe], input=" ".join(str(v) for v in words) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        return json.loads(r.stdout)

    return run


def test_commit_plan(commit_check):
    S = R.KE_SINGULAR
    out = commit_check(2, 6, 4, [
        # the common duplicate: the running chain's closest scan is the previous scan -> one edge, one constraint
        (0, 0, 3, [(4, 5, 0), (4, 5, 0), (1, 5, 0)]),
        # a -> b does not block b -> a; a singular record is skipped; record order is kept
        (0, 1, 4, [(2, 3, 0), (3, 2, 0), (0, 3, S), (2, 3, 0)]),
        # a job whose mean was singular still commits its records; a refused job has none (its row is garbage)
        (S, 0, 2, [(0, 5, 0), (4, 5, 0)]),
        (R.KE_ERANGE, 0, 3, []),
        (R.KE_EINVAL, 1, 0, []),
        # records beyond n_links are not read
        (0, 1, 1, [(0, 1, 0), (1, 0, 0)]),
    ])
    assert out["ok"] == 1
    assert out["actions"] == [[0, 0, 0, 4, 5, 1], [0, 1, 0, 4, 5, 0], [0, 2, 0, 1, 5, 1],
                              [1, 0, 1, 2, 3, 1], [1, 1, 1, 3, 2, 1], [1, 3, 1, 2, 3, 0],
                              [2, 0, 0, 0, 5, 1], [2, 1, 0, 4, 5, 0],
                              [5, 0, 1, 0, 1, 1]]
    assert out["edges"] == [[[4, 5], [1, 5], [0, 5]], [[2, 3], [3, 2], [0, 1]]]
    # the callback's refusal ends the plan; what went before stays
    out = commit_check(1, 4, 2, [(0, 0, 2, [(0, 1, 0), (2, 2, 0)]), (0, 0, 1, [(1, 2, 0)])])
    assert out["ok"] == 0 and out["actions"] == [[0, 0, 0, 0, 1, 1]] and out["edges"] == [[[0, 1]]]
    # the transcription's AddEdge agrees on a random stream
    rng = np.random.default_rng(8)
    recs = [tuple(int(v) for v in rng.choice(7, 2, replace=False)) + (0,) for _ in range(60)]
    out = commit_check(1, 7, 60, [(0, 0, 60, recs)])
    import karto_loop_plain as LP
    g = LP.Graph()
    for _ in range(7):
        g.add_vertex()
    assert [a[5] for a in out["actions"]] == [int(g.add_edge(f, t)[1]) for f, t, _ in recs]


# ------------------------------------------------------------------------------------ 4. the public interface
def test_abi_is_exported_and_layouts_match():
    hdr = open(os.path.join(REPO, "include", "slam2d", "karto_link.h")).read()
    names = sorted(set(re.findall(r"\b(ke_[a-z_]+)\s*\(", hdr)))
    assert len(names) >= 18 and {"ke_add_edges_device", "ke_loop_coarse_device", "ke_loop_fine_device", "ke_close_device",
                                 "ke_commit", "ke_get_loop_info", "ke_last_error", "ke_version", "ke_set_timing",
                                 "ke_num_kernels", "ke_kernel_name", "ke_get_kernel_times"} <= set(names)
    L = ke._lib.lib()
    ke._declare(L)
    for n in names:
        assert hasattr(L, n), f"{n} is declared in karto_link.h but not exported by libslam2d.so"
    assert ctypes.sizeof(ke.KeParams) == 32 and ctypes.sizeof(ke.KeJob) == 32 == R.JOB.itemsize
    assert ctypes.sizeof(ke.KeLink) == 112 == R.LINK.itemsize == ke.LINK_DTYPE.itemsize
    assert ctypes.sizeof(ke.KeJobOut) == 40 == R.JOB_OUT.itemsize == ke.JOB_OUT_DTYPE.itemsize
    assert ctypes.sizeof(ke.KeClosure) == 112 == R.CLOSURE.itemsize == ke.CLOSURE_DTYPE.itemsize
    assert R.KT_RESULT == kt.RESULT_DTYPE and R.CLOSEST == kl.CLOSEST_DTYPE and R.SOURCE == kl.SOURCE_DTYPE
    assert R.NEAR_CHAIN == kl.NEAR_CHAIN_DTYPE and R.LOOP_CHAIN == kl.LOOP_CHAIN_DTYPE and R.JOB == ke.JOB_DTYPE
    # the C compiler's layouts: the restatement is built from the same header
    assert [f for f, _ in ke.KeLink._fields_][:4] == ["from_", "to", "kind", "status"]
    for k in ("KE_MAX_LINKS", "KE_PREV", "KE_RUNNING", "KE_NEAR", "KE_LOOP", "KE_WRITE_POSE", "KE_LOOP_OVERFLOW",
              "KE_LOOP_EINVAL"):
        assert f"#define {k} {getattr(ke, k)}" in hdr, k
    assert "#define KE_ERANGE (-5)" in hdr and "#define KE_SINGULAR (-6)" in hdr and (ke.KE_ERANGE, ke.KE_SINGULAR) == (-5, -6)
    assert (R.KE_EINVAL, R.KE_ERANGE, R.KE_SINGULAR, R.KE_WRITE_POSE) == (ke.KE_EINVAL, ke.KE_ERANGE, ke.KE_SINGULAR, ke.KE_WRITE_POSE)
    assert L.ke_version().decode().startswith("slam2d-karto-link")
    kn = [L.ke_kernel_name(i).decode() for i in range(L.ke_num_kernels())]
    assert kn == ["ke_add_edges_kernel", "ke_coarse_scan_kernel", "ke_coarse_write_kernel", "ke_fine_kernel", "ke_close_kernel"]
    assert L.ke_kernel_name(-1) == b"" and L.ke_kernel_name(len(kn)) == b""
    import slam2d
    assert slam2d.LinkStage is ke.LinkStage


def test_params():
    d, n = ke.default_params(), ke.node_params()
    assert [getattr(d, k) for k, _ in ke.KeParams._fields_] == [0.8, 0.8, 0.4 * 0.4, 0.8]
    assert [getattr(n, k) for k, _ in ke.KeParams._fields_] == [0.1, 0.35, 9.0, 0.45]
    assert [getattr(d, k) for k in G.PARAM_KEYS] == [K.DEFAULT_PARAMS[k] for k in G.PARAM_KEYS]
    assert [getattr(n, k) for k in G.PARAM_KEYS] == [K.NODE_PARAMS[k] for k in G.PARAM_KEYS]
    assert ke.default_params(loop_match_minimum_response_fine=0.5).loop_match_minimum_response_fine == 0.5
    with pytest.raises(TypeError):
        ke.default_params(no_such_parameter=1)


def test_argument_refusals_need_no_device():
    L = ke._lib.lib()
    ke._declare(L)
    h = ctypes.c_void_p()
    p = ke.default_params()
    bad = [(None, (ctypes.byref(p), 360, 4, 64, 16), ke.KE_EINVAL, "out is NULL"),
           (h, (ctypes.byref(p), 0, 4, 64, 16), ke.KE_EINVAL, "n_readings"),
           (h, (ctypes.byref(p), 4097, 4, 64, 16), ke.KE_EINVAL, "n_readings"),
           (h, (ctypes.byref(p), 360, 0, 64, 16), ke.KE_EINVAL, "max_jobs"),
           (h, (ctypes.byref(p), 360, 4, 0, 16), ke.KE_EINVAL, "max_links"),
           (h, (ctypes.byref(p), 360, 4, 65, 16), ke.KE_ERANGE, "KE_MAX_LINKS"),
           (h, (ctypes.byref(p), 360, 4, 64, 0), ke.KE_EINVAL, "max_matches")]
    for out, args, code, word in bad:
        rc = L.ke_create(ctypes.byref(out) if out is not None else None, *args)
        assert rc == code and word in L.ke_last_error().decode(), (args, rc, L.ke_last_error())
        assert not h.value
    nanp = ke.default_params(loop_match_maximum_variance_coarse=math.nan)
    assert L.ke_create(ctypes.byref(h), ctypes.byref(nanp), 360, 4, 64, 16) == ke.KE_EINVAL
    # a NULL context is refused by every entry point, and destroying one is a no-op
    z = ctypes.c_int(0)
    assert L.ke_destroy(None) == 0
    assert L.ke_add_edges_device(None, 0, None, None, 1, None, 0, None, 0, None, None, 0, None, 0, 0, 0, None) == ke.KE_EINVAL
    assert L.ke_loop_coarse_device(None, 0, *([None] * 6), 1, 0, 0, 0, *([None] * 8)) == ke.KE_EINVAL
    assert L.ke_loop_fine_device(None, 0, 0, None, None, None, 0, None, None, None, 0, None, None, 0, 0, None) == ke.KE_EINVAL
    assert L.ke_close_device(None, 0, None, None, None, None, 1, None) == ke.KE_EINVAL
    assert L.ke_get_links(None, 0, 0, None, None) == ke.KE_EINVAL and L.ke_commit(None, None, None, 0, 0, ctypes.byref(z)) == ke.KE_EINVAL
    assert L.ke_get_loop_info(None, None, None) == ke.KE_EINVAL and L.ke_set_timing(None, 1) == ke.KE_EINVAL
    assert L.ke_result_device(None, None, None, None) == ke.KE_EINVAL and L.ke_get_kernel_times(None, None, None, 0) == ke.KE_EINVAL
    assert "ctx is NULL" in L.ke_last_error().decode()
