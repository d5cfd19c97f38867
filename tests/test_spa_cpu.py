"""The pose-graph optimiser without a GPU: the CPU restatement tests/ref/spa2d_ref.c (SysSPA2d::doSPA in its
block-Jacobi PCG mode) against closed forms and against the plain numpy LM tests/ref/spa2d_plain.py, the golden
fixture, the host helpers of slam2d.spa and the id lookup.  Eigen and SuiteSparse are absent, so parity with the
compiled sparse_bundle_adjustment is unpinned."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import spa2d_plain as P  # noqa: E402
import spa2d_ref as R  # noqa: E402

from slam2d import spa  # noqa: E402

K_DIAG = np.diag([100.0, 100.0, 400.0]).reshape(9)
# doSPA stops once a step is shorter than 1e-8 (sqMinDelta, spa2d.cpp:458), and PCG's abstol rule lets the last steps
# be inexact, so an optimum is reached to a few such steps, not to rounding: closed forms are compared within 1e-7.
ATOL = 1e-7
COST_ATOL = 6 * 400.0 * ATOL ** 2  # err' K err of at most two constraints' three components that far off


def test_closed_form_one_constraint():
    """One fixed node, one free node, one constraint: the optimum is fixed (+) mean, cost 0.  Fixed at (1, 2, pi/2),
    mean (0.5, -0.25, 0.3): the free node sits at (1 + 0.25, 2 + 0.5, pi/2 + 0.3) -- R(pi/2) (0.5, -0.25) =
    (0.25, 0.5)."""
    poses = [[1.0, 2.0, math.pi / 2.0], [0.0, 0.0, 0.0]]
    po, st = R.compute(poses, [[0, 1]], [[0.5, -0.25, 0.3]], [K_DIAG])
    assert st["status"] == R.OK and st["converged"] == 1 and st["lm_iters"] < 40
    np.testing.assert_array_equal(po[0], poses[0])
    np.testing.assert_allclose(po[1], [1.25, 2.5, math.pi / 2.0 + 0.3], rtol=0, atol=ATOL)
    assert st["final_cost"] < COST_ATOL < st["initial_cost"]


def test_closed_form_reversed_constraints():
    """Node 0 fixed at the origin; 2 -> 1 with mean (-1, 0, 0) and 1 -> 0 with mean (-1, 0, 0), both written from the
    higher index to the lower (i1 < i0: the transposed off-diagonal block, and the fixed node as nd1).  Consistent, so
    the optimum has cost 0: node 1 at (1, 0, 0), node 2 at (2, 0, 0).  A wrong sign or a missing transpose in the
    (1, 2) block leaves a residual or sends node 2 elsewhere."""
    poses = [[0.0, 0.0, 0.0], [0.7, 0.4, 0.2], [2.5, -0.3, -0.1]]
    ends = [[2, 1], [1, 0]]
    means = [[-1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]]
    po, st = R.compute(poses, ends, means, [K_DIAG, K_DIAG])
    assert st["status"] == R.OK and st["converged"] == 1
    np.testing.assert_allclose(po, [[0, 0, 0], [1, 0, 0], [2, 0, 0]], rtol=0, atol=ATOL)
    assert st["final_cost"] < COST_ATOL
    # the same graph by hand with rotated frames: 1 -> 0 seen from node 1 at heading pi/2 placed at (0, 1)
    poses = [[0.0, 0.0, 0.0], [0.1, 0.8, 1.2], [0.3, 2.2, 1.4]]
    means = [[-1.0, 0.0, 0.0], [-1.0, 0.0, -math.pi / 2.0]]
    po, st = R.compute(poses, ends, means, [K_DIAG, K_DIAG])
    assert st["converged"] == 1
    np.testing.assert_allclose(po, [[0, 0, 0], [0, 1, math.pi / 2.0], [0, 2, math.pi / 2.0]], rtol=0, atol=ATOL)


RING_SIZES = (6, 12, 33, 64)
# measured (this file, the cases below): largest pose deviation 2.80e-7 (64 nodes; 2.1e-8, 7.5e-9, 3.0e-8 at 6, 12,
# 33), largest relative cost deviation 8.2e-13 (64 nodes).  The bounds are ten times those.
POSE_BOUND = 2.8e-6
COST_BOUND = 8.3e-12


@pytest.mark.parametrize("n", RING_SIZES)
def test_restatement_against_plain_lm(n):
    """Ring graphs (two-hop links, one closure, drifted dead reckoning) at the reference's default parameters: the
    PCG-mode restatement ends by the convergence test before niter, and lands where an exact-solve LM lands.
    Measured: pose deviation 2.1e-8 / 7.5e-9 / 3.0e-8 / 2.8e-7 (m, rad) at 6 / 12 / 33 / 64 nodes, relative cost
    deviation 1.8e-13 / 2.4e-14 / 7.6e-14 / 8.2e-13; the bounds are ten times the largest (2.8e-6, 8.3e-12)."""
    c = R.case_ring(n, n)
    assert c["params"] == R.DEFAULTS
    po, st = R.compute_case(c)
    assert st["status"] == R.OK and st["converged"] == 1 and st["lm_iters"] < 40, st
    pp, ps = P.solve(c["poses"], c["ends"], c["means"], c["precs"])
    assert ps["converged"] == 1
    dev = float(np.abs(po - pp).max())
    rel = abs(st["final_cost"] - ps["final_cost"]) / ps["final_cost"]
    print(f"ring {n}: lm {st['lm_iters']} cg {st['cg_iters']} pose deviation {dev:.3e} relative cost deviation {rel:.3e}")
    assert dev <= POSE_BOUND and rel <= COST_BOUND, (dev, rel)
    assert st["initial_cost"] == pytest.approx(ps["initial_cost"], rel=1e-12)


def test_golden_fixture_reproduces_bit_for_bit():
    """The restatement on the fixture's stored inputs gives the stored poses and stats, every bit."""
    cases = R.load_golden()
    assert set(cases) == set(R.golden_cases())
    for name, (c, want_poses, want_stats) in cases.items():
        assert c["params"] == R.golden_cases()[name]["params"], name
        po, st = R.compute_case(c)
        R.assert_same_result(po, st, want_poses, want_stats, name)


def test_seeded_search_finds_the_rejecting_cases():
    """The graphs whose LM steps are undone come from a seeded search, not from luck: the first seed that rejects
    exactly once, the first that rejects exactly twice (lambda * 2, then * 4: laminc's doubling)."""
    s1, _, st1 = R.find_rejecting(1, 1)
    s2, _, st2 = R.find_rejecting(2, 2)
    assert (s1, s2) == (R.REJECT_ONCE_SEED, R.REJECT_TWICE_SEED)
    assert st1["rejected"] == 1 and st2["rejected"] == 2
    # every accepted step halves lambda, the rejections multiply it by 2, then by 4
    assert st1["lambda"] == 1e-4 * 0.5 ** st1["good_iter"] * 2.0
    assert st2["lambda"] == 1e-4 * 0.5 ** st2["good_iter"] * 8.0


def test_parameter_paths_of_the_restatement():
    """The bounds and branches the GPU cases rely on, seen through the stats."""
    c = R.case_ring(33, 5, max_cg_iters=2)
    _, st = R.compute_case(c, niter=1)
    assert st["cg_iters"] == 2  # the first PCG run (no abstol) ends at its bound, far from 1e-8
    _, st = R.compute_case(c)
    assert st["lm_iters"] == 40 and 40 < st["cg_iters"] <= 80 and st["converged"] == 0
    _, st = R.compute_case(R.case_ring(33, 6, niter=3))
    assert st["lm_iters"] == 3 and st["converged"] == 0
    c = R.case_ring(12, 7, init_tol=2.0)
    po, st = R.compute_case(c)  # dn < 2 dn at once: no PCG iteration, a zero step, convergence
    assert st["cg_iters"] == 0 and st["converged"] == 1 and st["lm_iters"] == 1 and st["good_iter"] == 0
    np.testing.assert_array_equal(po, c["poses"])
    _, st = R.compute_case(R.case_ring(12, 2))
    assert st["abstol_hits"] > 0  # the carried residual raised d0
    _, st = R.compute_case(R.case_ring(12, 4, n_fixed=0))
    assert st["status"] == R.NO_FIXED and st["lm_iters"] == 0
    c = R.case_disconnected()
    po, st = R.compute_case(c)
    assert st["status"] == R.DISCONNECTED
    np.testing.assert_array_equal(po, c["poses"])
    po, st = R.compute_case(R.case_empty())
    assert st["status"] == R.OK and st["good_iter"] == 0 and st["cg_iters"] == 0
    c = R.case_near_pi()
    po, st = R.compute_case(c)
    assert np.any(np.sign(po[:, 2]) != np.sign(c["poses"][:, 2]))  # a heading crossed +-pi: normArot fired
    assert np.abs(po[:, 2]).max() <= math.pi


def test_id_lookup_semantics():
    """addConstraint (spa2d.cpp:230-252): an unknown id returns false and adds nothing; of two nodes with one id the
    LAST wins."""
    g = R.RefGraph()
    g.add_node(7, [0, 0, 0])
    g.add_node(9, [1, 0, 0])
    g.add_node(9, [2, 0, 0])
    assert g.add_constraint(7, 8, [1, 0, 0], K_DIAG) is False and g.ends == []
    assert g.add_constraint(7, 9, [2, 0, 0], K_DIAG) is True
    assert g.ends == [[0, 2]]
    assert g.add_constraint(9, 7, [-2, 0, 0], K_DIAG) is True and g.ends[-1] == [2, 0]


def test_matrix3_inverse_helper():
    """Matrix3::Inverse by cofactors (Karto.h:2445-2490) on a hand-inverted matrix: [[2, 0, 0], [0, 4, 2], [0, 2, 2]]
    has determinant 8 and inverse [[0.5, 0, 0], [0, 0.5, -0.5], [0, -0.5, 1]]."""
    got = spa.matrix3_inverse([[2, 0, 0], [0, 4, 2], [0, 2, 2]])
    np.testing.assert_array_equal(got, [[0.5, 0, 0], [0, 0.5, -0.5], [0, -0.5, 1.0]])
    with pytest.raises(spa.Slam2dError):
        spa.matrix3_inverse(np.zeros((3, 3)))
    k = spa.precision_of(np.diag([0.25, 0.5, 0.125]))
    np.testing.assert_array_equal(k, np.diag([4.0, 2.0, 8.0]))


def test_link_info_helper():
    """LinkInfo::Update (Mapper.h:138-152).  Pose 1 at (1, 1, pi/2), pose 2 at (1, 3, pi): seen from pose 1 the
    second lies 2 m ahead, turned by pi/2.  The covariance diag(4, 1, 9) turns by -pi/2: x and y variances swap."""
    mean, cov = spa.link_info([1.0, 1.0, math.pi / 2.0], [1.0, 3.0, math.pi], np.diag([4.0, 1.0, 9.0]))
    np.testing.assert_allclose(mean, [2.0, 0.0, math.pi / 2.0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(cov, np.diag([1.0, 4.0, 9.0]), rtol=0, atol=1e-14)
    # from the origin the transform is the identity (SetTransform's shortcut)
    mean, cov = spa.link_info([0.0, 0.0, 0.0], [0.5, -0.25, 4.0], np.eye(3))
    np.testing.assert_array_equal(mean, [0.5, -0.25, 4.0 - 2.0 * math.pi])
    assert spa.normalize_angle(-4.0) == -4.0 + 2.0 * math.pi and spa.normalize_angle(1.0) == 1.0
