"""The pose-graph optimiser's direct mode without a GPU: the restatement tests/ref/spa2d_chol_ref.c (SysSPA2d::doSPA
with the envelope Cholesky solve include/slam2d/spa.h states) -- its solve against numpy within the backward-error
bound of a Cholesky solve, the envelope rule on hand-counted graphs (through a stand-alone C++ host of
csrc/spa_graph.h built with -fsanitize=address,undefined), the whole compute against the plain numpy LM
tests/ref/spa2d_plain.py and against closed forms, the golden fixture and the statuses.  SuiteSparse is absent:
cs_cholsol's own order, its AMD permutation and CHOLMOD are unpinned."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "ref"))
import spa2d_chol_ref as CH  # noqa: E402
import spa2d_plain as P  # noqa: E402
import spa2d_ref as R  # noqa: E402

from slam2d import spa  # noqa: E402

K_DIAG = np.diag([100.0, 100.0, 400.0]).reshape(9)
ATOL = 1e-7  # tests/test_spa_cpu.py's: doSPA stops once a step is shorter than 1e-8
COST_ATOL = 6 * 400.0 * ATOL ** 2


# ------------------------------------------------------------------------------------------- 1. the solve alone
def _first(nb, shape):
    first = np.maximum(np.arange(nb) - 2, 0)  # a banded chain: two blocks back
    if shape == "full_row":
        first[nb - 1] = 0
    elif shape == "hub":
        h = nb // 3
        first[h + 1::2] = np.minimum(first[h + 1::2], h)  # every other row above the hub reaches back to it
    return first.astype(np.int32)


def _spd(nb, shape, seed):
    """A = M M' for a random M with the envelope's structure: M M' stays inside the envelope."""
    rng = np.random.default_rng(seed)
    first = _first(nb, shape)
    n = 3 * nb
    M = np.zeros((n, n))
    for k in range(nb):
        for c in range(3):
            i = 3 * k + c
            M[i, 3 * first[k]:i] = rng.normal(0.0, 0.3, i - 3 * first[k])
            M[i, i] = rng.uniform(1.0, 2.0)
    A = np.tril(M @ M.T)
    return first, A + np.tril(A, -1).T, rng.normal(0.0, 1.0, n)  # exactly symmetric


def _gamma(k):
    u = 2.0 ** -53
    return k * u / (1.0 - k * u)


@pytest.mark.parametrize("shape", ["band", "full_row", "hub"])
@pytest.mark.parametrize("nb", [1, 2, 10, 33, 100])
def test_chol_solve_against_numpy(nb, shape):
    """N = 3 nb = 3, 6, 30, 99, 300 scalars.  Bound (derived, not measured): a Cholesky solve computes x with
    (A + dA) x = b, |dA| <= gamma_{3N+1} |R'||R| (Higham, Accuracy and Stability, Thm 10.4), and || |R'||R| ||_2 <=
    N ||A||_2 (Lemma 6.6 with ||R||_2^2 = ||A||_2), so ||A x - b||_2 <= N gamma_{3N+1} ||A||_2 ||x||_2."""
    first, A, b = _spd(nb, shape, 100 * nb + len(shape))
    N = 3 * nb
    x, ok, L_env = CH.chol_solve(first, CH.pack_env(A, first), b)
    assert ok
    res = float(np.linalg.norm(A @ x - b))
    bound = N * _gamma(3 * N + 1) * float(np.linalg.norm(A, 2)) * float(np.linalg.norm(x))
    print(f"N {N} {shape}: residual {res:.3e} bound {bound:.3e}")
    assert res <= bound
    # the factor: inside the envelope by its storage; it is A's factor (Thm 10.3: |A - L L'| <= gamma_{N+1} |L||L'|),
    # and the dense factor of the same matrix has nothing outside the envelope either
    L = CH.unpack_env(L_env, first)
    assert np.all(np.abs(A - L @ L.T) <= _gamma(N + 1) * (np.abs(L) @ np.abs(L.T)))
    outside = np.ones((N, N), bool)
    for k in range(nb):
        for c in range(3):
            outside[3 * k + c, 3 * first[k]:3 * k + c + 1] = False
    assert np.all(np.linalg.cholesky(A)[outside] == 0.0)
    np.testing.assert_allclose(x, np.linalg.solve(A, b), rtol=0,
                               atol=2 * N * _gamma(3 * N + 1) * np.linalg.cond(A) * np.linalg.norm(x))


@pytest.mark.parametrize("nb", [1, 10, 33])
def test_chol_solve_refuses_a_negative_eigenvalue(nb):
    first, A, b = _spd(nb, "hub", 7 * nb)
    A = A - (np.linalg.eigvalsh(A)[0] + 0.5) * np.eye(3 * nb)  # the smallest eigenvalue becomes -0.5
    x, ok, _ = CH.chol_solve(first, CH.pack_env(A, first), b)
    assert not ok and np.all(np.isnan(x))  # x is not written
    A[0, 0] = float("nan")
    assert not CH.chol_solve(first, CH.pack_env(A, first), b)[1]


# ------------------------------------------------------------------------------------------- 2. the envelope rule
@pytest.fixture(scope="module")
def envelope_check(tmp_path_factory):
    """tests/cpp/spa_envelope_check.cpp under ASan + UBSan, as its header says; a stand-alone program."""
    exe = str(tmp_path_factory.mktemp("spa_env") / "spa_envelope_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=all", "-I",
                    R.CSRC, os.path.join(HERE, "cpp", "spa_envelope_check.cpp"), "-o", exe], check=True)

    def run(n, n_fixed, links):
        line = " ".join(str(v) for v in [n, n_fixed, len(links)] + [e for ab in links for e in ab]) + "\n"
        out = subprocess.run([exe], input=line, capture_output=True, text=True, check=True).stdout
        return json.loads(out)

    return run


CHAIN5 = [(0, 1), (1, 2), (2, 3), (3, 4)]
ENVELOPES = {
    # name: (n, n_fixed, links, first per free node (node indices), blocks) -- counted by hand
    "chain": (5, 1, CHAIN5, [1, 1, 2, 3], 1 + 2 + 2 + 2),
    # node 4 also reaches back to node 1, the first free one: its row spans all four free nodes
    "closure": (5, 1, CHAIN5 + [(4, 1)], [1, 1, 2, 1], 1 + 2 + 2 + 4),
    "closure_reversed_repeated": (5, 1, [(b, a) for a, b in CHAIN5] + [(1, 4), (4, 1), (2, 1)], [1, 1, 2, 1], 9),
    # n_fixed = 2; node 4's only neighbours are the fixed nodes 0 and 1: first = itself
    "fixed_only": (5, 2, [(0, 1), (1, 2), (2, 3), (0, 4), (4, 1)], [2, 2, 4], 1 + 2 + 1),
    "chain_fixed2": (5, 2, CHAIN5, [2, 2, 3], 1 + 2 + 2),
    # a higher free neighbour does not count: node 1 is tied to 3 only, node 3 to 1 and 2
    "upward": (4, 1, [(0, 1), (1, 3), (0, 2), (2, 3)], [1, 2, 1], 1 + 1 + 3),
    "nothing_fixed": (3, 0, [(0, 1), (1, 2)], [], 0),
    "all_fixed": (3, 5, [(0, 1), (1, 2)], [], 0),
}


@pytest.mark.parametrize("name", list(ENVELOPES))
def test_envelope_rule_on_hand_counted_graphs(envelope_check, name):
    n, n_fixed, links, first, blocks = ENVELOPES[name]
    assert envelope_check(n, n_fixed, links) == {"first": first, "blocks": blocks}
    if n_fixed > 0:  # the restatement's scatter form of the rule (free indices) agrees
        got = CH.first_of(n, links, n_fixed)
        assert (got + min(n_fixed, n)).tolist() == first
        assert int(np.sum(np.arange(len(got)) - got + 1)) == blocks


# ------------------------------------------------------------------------------------------- 3. against the plain LM
RING_SIZES = (6, 12, 33, 64)
# measured (this file, the cases below): largest pose deviation 2.6e-9 (33 nodes; 4.4e-16, 4.4e-16, 5.6e-16 at 6, 12,
# 64), largest relative cost deviation 6.7e-15 (6 nodes; 4.2e-15, 2.6e-15, 1.2e-15 at 12, 33, 64).  The bounds are ten
# times those, the margin tests/test_spa_cpu.py uses for the PCG mode (whose bounds are 2.8e-6 and 8.3e-12).
POSE_BOUND = 2.6e-8
COST_BOUND = 6.7e-14
# the rings on which the restatement's lm_iters, good_iter and rejected equal the plain LM's.  At 33 nodes both run 9
# iterations, but from the fifth on the steps are 1.2e-8 long and move the cost by less than its last two bits: the
# restatement (256-lane sum) undoes four of them, the plain LM (sequential sum) undoes three and accepts one on a fall
# of 5 ulp.
SAME_COUNTS = (6, 12, 64)


def _deviation(c):
    po, st = CH.compute_case(c)
    pp, ps = P.solve(c["poses"], c["ends"], c["means"], c["precs"])
    dev = float(np.abs(po - pp).max())
    rel = abs(st["final_cost"] - ps["final_cost"]) / ps["final_cost"]
    return st, ps, dev, rel


@pytest.mark.parametrize("n", RING_SIZES)
def test_restatement_against_plain_lm(n):
    """Ring graphs at the reference's default parameters: the direct-mode restatement converges and lands where the
    exact-solve LM lands.  Measured: pose deviation 4.4e-16 / 4.4e-16 / 2.6e-9 / 5.6e-16 (m, rad) at 6 / 12 / 33 / 64
    nodes, relative cost deviation 6.7e-15 / 4.2e-15 / 2.6e-15 / 1.2e-15; the bounds are ten times the largest.  LM
    iterations / accepted / rejected: 4/3/0, 5/4/0, 9/4/4 (plain 9/5/3), 7/6/0."""
    c = R.case_ring(n, n)
    assert c["params"] == R.DEFAULTS
    st, ps, dev, rel = _deviation(c)
    print(f"ring {n}: lm {st['lm_iters']} good {st['good_iter']} rejected {st['rejected']} | plain lm {ps['lm_iters']} "
          f"good {ps['good_iter']} rejected {ps['rejected']} | pose deviation {dev:.3e} relative cost deviation {rel:.3e}")
    assert st["status"] == CH.OK and st["converged"] == 1 and st["cg_iters"] == 0, st
    assert ps["converged"] == 1
    if n in SAME_COUNTS:
        assert [st[k] for k in ("lm_iters", "good_iter", "rejected")] == [ps[k] for k in ("lm_iters", "good_iter", "rejected")]
    assert dev <= POSE_BOUND and rel <= COST_BOUND, (dev, rel)
    assert st["initial_cost"] == pytest.approx(ps["initial_cost"], rel=1e-12)


# ------------------------------------------------------------------------------------------- 4. what the mode is for
def test_growing_radius_ring_converges():
    """The ring of radius 9.6 m at 64 nodes: the PCG mode uses all 40 LM iterations and stops 2e-3 from the exact-step
    LM; the direct mode converges before niter, within the ring bound.  Measured: 13 LM iterations (8 accepted, 4
    undone; the plain LM takes 10), pose deviation 8.1e-9, relative cost deviation 5.8e-15."""
    c = CH.grown_ring(64, 64)
    assert float(np.hypot(c["poses"][0, 0], c["poses"][0, 1])) == pytest.approx(9.6)
    pr, sr = R.compute_case(c)
    st, ps, dev, rel = _deviation(c)
    pcg_dev = float(np.abs(pr - P.solve(c["poses"], c["ends"], c["means"], c["precs"])[0]).max())
    print(f"grown ring: lm {st['lm_iters']} good {st['good_iter']} rejected {st['rejected']} | plain lm {ps['lm_iters']} | "
          f"pose deviation {dev:.3e} relative cost deviation {rel:.3e} | PCG lm {sr['lm_iters']} deviation {pcg_dev:.3e}")
    assert sr["converged"] == 0 and sr["lm_iters"] == 40 and pcg_dev > 1e-3  # the gap this mode closes
    assert st["status"] == CH.OK and st["converged"] == 1 and st["lm_iters"] < c["params"]["niter"], st
    assert dev <= POSE_BOUND and rel <= COST_BOUND, (dev, rel)


# ------------------------------------------------------------------------------------------- 5. closed forms
def test_closed_form_one_constraint():
    """tests/test_spa_cpu.py's case: fixed at (1, 2, pi/2), mean (0.5, -0.25, 0.3): the free node sits at
    (1.25, 2.5, pi/2 + 0.3), cost 0."""
    poses = [[1.0, 2.0, math.pi / 2.0], [0.0, 0.0, 0.0]]
    po, st = CH.compute(poses, [[0, 1]], [[0.5, -0.25, 0.3]], [K_DIAG])
    assert st["status"] == CH.OK and st["converged"] == 1 and st["lm_iters"] < 40
    np.testing.assert_array_equal(po[0], poses[0])
    np.testing.assert_allclose(po[1], [1.25, 2.5, math.pi / 2.0 + 0.3], rtol=0, atol=ATOL)
    assert st["final_cost"] < COST_ATOL < st["initial_cost"]


def test_closed_form_reversed_constraints():
    """tests/test_spa_cpu.py's case: 2 -> 1 and 1 -> 0, both written from the higher index to the lower (the
    transposed pair block enters the envelope), consistent, so the optimum has cost 0; then with rotated frames."""
    poses = [[0.0, 0.0, 0.0], [0.7, 0.4, 0.2], [2.5, -0.3, -0.1]]
    ends = [[2, 1], [1, 0]]
    means = [[-1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]]
    po, st = CH.compute(poses, ends, means, [K_DIAG, K_DIAG])
    assert st["status"] == CH.OK and st["converged"] == 1
    np.testing.assert_allclose(po, [[0, 0, 0], [1, 0, 0], [2, 0, 0]], rtol=0, atol=ATOL)
    assert st["final_cost"] < COST_ATOL
    poses = [[0.0, 0.0, 0.0], [0.1, 0.8, 1.2], [0.3, 2.2, 1.4]]
    means = [[-1.0, 0.0, 0.0], [-1.0, 0.0, -math.pi / 2.0]]
    po, st = CH.compute(poses, ends, means, [K_DIAG, K_DIAG])
    assert st["converged"] == 1
    np.testing.assert_allclose(po, [[0, 0, 0], [0, 1, math.pi / 2.0], [0, 2, math.pi / 2.0]], rtol=0, atol=ATOL)


# ------------------------------------------------------------------------------------------- 6. fixture and statuses
def test_golden_fixture_reproduces_bit_for_bit():
    cases = CH.load_golden()
    assert set(cases) == set(CH.golden_cases())
    for name, (c, want_poses, want_stats) in cases.items():
        fresh = CH.golden_cases()[name]
        assert c["params"] == fresh["params"], name
        np.testing.assert_array_equal(R.bits(c["poses"]), R.bits(fresh["poses"]), err_msg=name)
        po, st = CH.compute_case(c)
        R.assert_same_result(po, st, want_poses, want_stats, name)
    assert cases["not_posdef"][2]["status"] == CH.NOT_POSDEF and cases["reject2"][2]["rejected"] == 2


def test_seeded_search_finds_the_rejecting_cases():
    """The search of spa2d_ref.find_rejecting, run again for this mode."""
    s1, _, st1 = CH.find_rejecting(1, 1)
    s2, _, st2 = CH.find_rejecting(2, 2)
    assert (s1, s2) == (CH.REJECT_ONCE_SEED, CH.REJECT_TWICE_SEED)
    assert st1["lambda"] == 1e-4 * 0.5 ** st1["good_iter"] * 2.0
    assert st2["lambda"] == 1e-4 * 0.5 ** st2["good_iter"] * 8.0


def test_solver_selection_and_statuses():
    p = spa.default_params()
    assert p.solver == spa.SPA_SOLVER_PCG == 0 and C_sizeof(p) == 32
    assert spa.default_params(solver="cholesky").solver == spa.SPA_SOLVER_CHOLESKY == 1
    assert spa.default_params(solver="pcg").solver == 0 and spa.default_params(solver=1).solver == 1
    for bad in (7, -1, "direct"):
        with pytest.raises(ValueError):
            spa.default_params(solver=bad)
    assert (spa.SPA_NOT_POSDEF, spa.SPA_FACTOR_RANGE) == (CH.NOT_POSDEF, CH.FACTOR_RANGE) == (3, 4)
    # a constraint with precision -I: refused on the first factor, poses as they came, stats to date
    c = CH.case_not_posdef()
    po, st = CH.compute_case(c)
    assert st["status"] == CH.NOT_POSDEF and (st["lm_iters"], st["good_iter"], st["converged"]) == (1, 0, 0)
    np.testing.assert_array_equal(R.bits(po), R.bits(c["poses"]))
    assert st["final_cost"] == st["initial_cost"] and st["lambda"] == 1e-4
    # capacity: the envelope's own block count runs, one block less is refused with the poses untouched
    c = CH.case_full_row()
    blocks = CH.envelope_blocks(c)
    assert blocks == 1 + 2 + 3 * 36 + 39
    assert CH.compute_case(c, max_factor_blocks=blocks)[1]["status"] == CH.OK
    po, st = CH.compute_case(c, max_factor_blocks=blocks - 1)
    assert st["status"] == CH.FACTOR_RANGE and st["lm_iters"] == 0
    np.testing.assert_array_equal(R.bits(po), R.bits(c["poses"]))
    assert CH.compute_case(R.case_ring(12, 4, n_fixed=0))[1]["status"] == CH.NO_FIXED
    assert CH.compute_case(R.case_disconnected())[1]["status"] == CH.DISCONNECTED
    po, st = CH.compute_case(R.case_empty(), max_factor_blocks=0)
    assert st["status"] == CH.OK and st["converged"] == 1


def C_sizeof(p):
    import ctypes

    return ctypes.sizeof(p)
