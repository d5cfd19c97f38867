"""GPU parity of the pose-graph optimiser's direct mode (spa_solve_kernel<SPA_SOLVER_CHOLESKY>: SysSPA2d::doSPA with
the envelope Cholesky solve include/slam2d/spa.h states) against the CPU restatement tests/ref/spa2d_chol_ref.c.  Bar:
bit-exact -- every pose's bits, the bits of the initial and final cost and of lambda, every integer of the stats.  The
restatement factors scalar by scalar, row by row; the kernel factors by block column with a lane per row, solves
forward inside the factor and backward by block row, so the schedule is under test.  The context's scratch (the
factor and the envelope's index arrays included) is poisoned before each launch.  SuiteSparse is absent: parity with
cs_cholsol / CHOLMOD is unpinned.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import karto_grid_ref as KG  # noqa: E402
import spa2d_chol_ref as CH  # noqa: E402
import spa2d_plain as P  # noqa: E402
import spa2d_ref as R  # noqa: E402

from slam2d import karto, karto_grid, spa  # noqa: E402
from slam2d.spa import SpaFleet  # noqa: E402

pytestmark = pytest.mark.gpu

K_DIAG = np.diag([100.0, 100.0, 400.0]).reshape(9)


def case_zero_step() -> dict:
    """Poses that meet every constraint exactly (err = 0 in every component): B = 0, the step is 0, convergence on the
    first iteration with nothing accepted."""
    poses = [[float(k), 0.0, 0.0] for k in range(5)]
    links = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 2)]
    means = [[float(b - a), 0.0, 0.0] for a, b in links]
    return R._case(poses, links, means, [K_DIAG] * len(links))


def case_chain_plus_leaf(leaf: bool) -> dict:
    """Ten free nodes in a two-hop chain: 1 + 2 + 3 * 8 = 27 blocks; with the leaf, an eleventh free node tied to the
    fixed node only: 28."""
    n = 12 if leaf else 11
    rng = np.random.default_rng(51)
    truth = np.stack([0.5 * np.arange(n), 0.3 * np.sin(0.2 * np.arange(n)), 0.1 * np.sin(0.1 * np.arange(n))], axis=1)
    links = [(i, i + 1) for i in range(10)] + [(i, i + 2) for i in range(9)] + ([(0, 11)] if leaf else [])
    return R.graph_from_truth(truth, links, rng)


CASES = {
    # free-node counts 1, 2, 3, and the lane strides of the per-node loops
    "free1": lambda: CH.case_two_hop_chain(1, 61), "free2": lambda: CH.case_two_hop_chain(2, 62),
    "free3": lambda: CH.case_two_hop_chain(3, 63), "free255": lambda: CH.case_two_hop_chain(255, 64),
    "free256": lambda: CH.case_two_hop_chain(256, 65), "free257": lambda: CH.case_two_hop_chain(257, 66),
    "free513": lambda: CH.case_two_hop_chain(513, 67),
    # shapes of the envelope
    "full_row": CH.case_full_row, "mid": CH.case_mid_closures,
    "hub_low": lambda: R.case_hub(seed=11, n=90, hub=25), "hub_high": lambda: R.case_hub(seed=16, n=90, hub=65),
    "fixed_only": CH.case_fixed_only, "fixed2": lambda: R.case_ring(12, 4, n_fixed=2),
    "fixed2_chain": lambda: CH.case_two_hop_chain(20, 68, n_fixed=2),
    "reversed": R.case_reversed, "repeated": R.case_repeated, "near_pi": R.case_near_pi,
    # control paths
    "reject1": lambda: R.case_outliers(CH.REJECT_ONCE_SEED), "reject2": lambda: R.case_outliers(CH.REJECT_TWICE_SEED),
    "niter1": lambda: R.case_ring(33, 6, niter=1), "niter3": lambda: R.case_ring(33, 6, niter=3),
    "zero_step": case_zero_step, "ring33": lambda: R.case_ring(33, 33), "not_posdef": CH.case_not_posdef,
}


@functools.lru_cache(maxsize=None)
def _want(name):
    """A named case and the restatement's result, computed once and shared (treat as read-only)."""
    c = CASES[name]()
    po, st = CH.compute_case(c)
    return c, po, st


def _params(prm: dict, solver="cholesky") -> spa.SpaParams:
    return spa.default_params(solver=solver, **prm)


def _fleet(cases, extra=0, blocks=None) -> SpaFleet:
    n = max(len(c["poses"]) for c in cases)
    m = max(len(c["ends"]) for c in cases)
    if blocks is None:  # the largest envelope exactly: a block written past a graph's factor lands in the next graph's
        blocks = max(CH.envelope_blocks(c) for c in cases)
    return SpaFleet(len(cases) + extra, n + 3, m + 5, blocks)


def _load(f, g, c):
    f.set_graph(g, c["ids"], c["poses"], c["ends"], c["means"], c["precs"])


def _result(f, g):
    ids, poses = f.get_nodes(g)
    return ids, poses, f.stats(g)


@pytest.mark.parametrize("name", list(CASES))
def test_case_against_restatement(gpu, name):
    c, want_poses, want_stats = _want(name)
    f = _fleet([c])
    _load(f, 0, c)
    assert f.envelope_blocks(0, c["params"]["n_fixed"]) == CH.envelope_blocks(c) == f.max_factor_blocks
    f.poison_scratch(0xFF)  # NaN doubles, -1 indices: a value read before it is written spreads
    f.compute(0, 1, _params(c["params"]))
    ids, poses, st = _result(f, 0)
    np.testing.assert_array_equal(ids, c["ids"])
    assert st["cg_iters"] == 0
    R.assert_same_result(poses, st, want_poses, want_stats, name)
    f.close()


def test_the_cases_take_the_paths_they_are_named_for(gpu):
    """What the restatement's stats and the envelope rule say about the cases above."""
    assert _want("reject1")[2]["rejected"] == 1 and _want("reject2")[2]["rejected"] == 2
    assert _want("ring33")[2]["rejected"] == 4  # the rejections of tests/test_spa_chol_cpu.py's ring
    assert (_want("niter1")[2]["lm_iters"], _want("niter1")[2]["converged"]) == (1, 0)
    assert (_want("niter3")[2]["lm_iters"], _want("niter3")[2]["converged"]) == (3, 0)
    st = _want("zero_step")[2]
    assert (st["lm_iters"], st["good_iter"], st["converged"], st["initial_cost"]) == (1, 0, 1, 0.0)
    np.testing.assert_array_equal(_want("zero_step")[1], _want("zero_step")[0]["poses"])
    assert _want("not_posdef")[2]["status"] == CH.NOT_POSDEF
    for name, free in (("free1", 1), ("free2", 2), ("free3", 3), ("free255", 255), ("free256", 256), ("free257", 257),
                       ("free513", 513)):
        c = _want(name)[0]
        assert len(c["poses"]) - c["params"]["n_fixed"] == free and _want(name)[2]["status"] == CH.OK
        assert CH.envelope_blocks(c) == ((1, 3)[free - 1] if free < 3 else 3 * free - 3)
    c = _want("full_row")[0]
    assert CH.first_of(40, c["ends"], 1)[-1] == 0  # the last row starts at the first free node
    first = CH.first_of(60, _want("mid")[0]["ends"], 1)
    assert first[49] == 19 and first[54] == 20 and first[43] == 8 and first[50] == 48  # far back, between short rows
    for name, hub in (("hub_low", 25), ("hub_high", 65)):
        c = _want(name)[0]
        nb = {int(b if a == hub else a) for a, b in c["ends"] if hub in (a, b)}
        assert len(nb) == 40 and sum(v < hub for v in nb) == 20
    c = _want("fixed_only")[0]
    assert c["params"]["n_fixed"] == 2 and CH.first_of(8, c["ends"], 2).tolist() == [0, 0, 2, 1, 0, 3]
    assert all(a > b for a, b in _want("reversed")[0]["ends"])
    c, po, _ = _want("near_pi")
    assert np.all(np.abs(np.abs(c["poses"][:, 2]) - np.pi) < 1e-1) and np.any(np.sign(po[:, 2]) != np.sign(c["poses"][:, 2]))


def test_fleet_statuses_in_one_launch(gpu):
    """One launch: OK graphs, SPA_NO_FIXED, SPA_DISCONNECTED, SPA_NOT_POSDEF and SPA_FACTOR_RANGE.  The context holds
    27 blocks per graph: the two-hop chain of ten free nodes fills it exactly and runs, the same chain with a leaf
    needs 28 and is refused with its poses untouched.  n_fixed differs across the fleet."""
    cases = [case_chain_plus_leaf(False), case_chain_plus_leaf(True), R.case_ring(9, 3), R.case_disconnected(),
             CH.case_not_posdef(), R.case_ring(9, 5), CH.case_fixed_only(), R.case_empty()]
    n_fixed = [None, None, 0, None, None, 2, 2, None]
    want_status = [spa.SPA_OK, spa.SPA_FACTOR_RANGE, spa.SPA_NO_FIXED, spa.SPA_DISCONNECTED, spa.SPA_NOT_POSDEF,
                   spa.SPA_OK, spa.SPA_OK, spa.SPA_OK]
    f = _fleet(cases, blocks=27)
    for g, (c, nf) in enumerate(zip(cases, n_fixed)):
        _load(f, g, c)
        f.set_n_fixed(g, nf)
        assert f.envelope_blocks(g, 1 if nf is None else nf) == (CH.envelope_blocks(c, 1 if nf is None else nf) if nf != 0 else 0)
    assert f.envelope_blocks(0, 1) == 27 and f.envelope_blocks(1, 1) == 28
    f.poison_scratch(0xFF)
    f.compute(0, len(cases), _params(R.DEFAULTS))
    got = [_result(f, g) for g in range(len(cases))]
    f.close()
    assert [s["status"] for _, _, s in got] == want_status
    for g, (c, nf) in enumerate(zip(cases, n_fixed)):
        po, st = CH.compute_case(c, max_factor_blocks=27, **({} if nf is None else {"n_fixed": nf}))
        R.assert_same_result(got[g][1], got[g][2], po, st, f"graph {g}")
    for g in (1, 2, 3, 4):  # refused graphs keep their poses
        np.testing.assert_array_equal(R.bits(got[g][1]), R.bits(cases[g]["poses"]))
    # without factor storage every graph with a free node is refused; the PCG mode on the same context still runs
    f = _fleet(cases[:1], blocks=0)
    _load(f, 0, cases[0])
    f.compute(0, 1, _params(R.DEFAULTS))
    _, poses, st = _result(f, 0)
    assert st["status"] == spa.SPA_FACTOR_RANGE
    np.testing.assert_array_equal(R.bits(poses), R.bits(cases[0]["poses"]))
    f.compute(0, 1, _params(R.DEFAULTS, "pcg"))
    R.assert_same_result(*_result(f, 0)[1:], *R.compute_case(cases[0]), "pcg, no factor storage")
    f.close()


def test_compute_grow_compute_and_poison(gpu):
    """Poses persist: compute, poison, compute again; then grow the graph by id (the envelope changes: the new node
    closes back to node 2) and compute, each against the restatement doing the same."""
    c = _want("ring33")[0]
    f = SpaFleet(1, 40, 90, 200)
    for i, p in zip(c["ids"], c["poses"]):
        f.add_node(0, int(i), p)
    for (a, b), z, k in zip(c["ends"], c["means"], c["precs"]):
        assert f.add_constraint(0, int(c["ids"][a]), int(c["ids"][b]), z, k) is True
    prm = _params(R.DEFAULTS)
    f.poison_scratch(0xFF)
    f.compute(0, 1, prm)
    _, poses, got = _result(f, 0)
    R.assert_same_result(poses, got, *_want("ring33")[1:], "first")
    po2, st2 = CH.compute(_want("ring33")[1], c["ends"], c["means"], c["precs"])
    f.poison_scratch(0xFF)
    f.compute(0, 1, prm)
    _, poses, got = _result(f, 0)
    R.assert_same_result(poses, got, po2, st2, "second, from the first's poses, after poison")
    rng = np.random.default_rng(8)
    new_poses = np.array([[0.3, 2.1, 3.0], [-0.4, 2.0, -2.9]])
    links = [(32, 33), (33, 34), (34, 2), (31, 33)]
    zs, ks = [rng.normal(0.0, 0.3, 3) for _ in links], [R.random_prec(rng) for _ in links]
    for i, p in zip((700, 701), new_poses):
        f.add_node(0, i, p)
    ids = list(c["ids"]) + [700, 701]
    for (a, b), z, k in zip(links, zs, ks):
        assert f.add_constraint(0, ids[a], ids[b], z, k) is True
    assert f.envelope_blocks(0, 1) == CH.envelope_blocks(c) + 3 + 33  # rows 31 .. 33 and 2 .. 34
    po3, st3 = CH.compute(np.vstack([po2, new_poses]), np.vstack([c["ends"], links]), np.vstack([c["means"], zs]),
                          np.vstack([c["precs"], ks]))
    f.poison_scratch(0xFF)
    f.compute(0, 1, prm)
    _, poses, got = _result(f, 0)
    assert st3["status"] == CH.OK and st3["good_iter"] > 0
    R.assert_same_result(poses, got, po3, st3, "grown")
    f.close()


def test_pcg_then_cholesky_on_one_context(gpu):
    c = _want("mid")[0]
    f = _fleet([c])
    _load(f, 0, c)
    f.poison_scratch(0xFF)
    f.compute(0, 1, _params(c["params"], "pcg"))
    R.assert_same_result(*_result(f, 0)[1:], *R.compute_case(c), "pcg")
    _load(f, 0, c)
    f.compute(0, 1, _params(c["params"]))
    R.assert_same_result(*_result(f, 0)[1:], *_want("mid")[1:], "cholesky after pcg")
    _load(f, 0, c)
    f.compute(0, 1, _params(c["params"], "pcg"))
    R.assert_same_result(*_result(f, 0)[1:], *R.compute_case(c), "pcg after cholesky")
    f.close()


def test_nan_pose_ends_and_the_others_are_exact(gpu):
    """A NaN in one pose of the middle graph: its first pivot test fails (NaN is not > 0) or its loops end by their
    bounds; either way it equals the restatement (counters, status, untouched poses; NaN costs compared as NaN), and
    its neighbours in the launch are exact."""
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _want("full_row")[0].items()}
    bad["poses"][17, 1] = float("nan")
    cases = [_want("mid")[0], bad, _want("hub_low")[0]]
    f = _fleet(cases)
    for g, c in enumerate(cases):
        _load(f, g, c)
    f.poison_scratch(0xFF)
    f.compute(0, 3, _params(R.DEFAULTS))
    R.assert_same_result(*_result(f, 0)[1:], *_want("mid")[1:], "graph 0")
    R.assert_same_result(*_result(f, 2)[1:], *_want("hub_low")[1:], "graph 2")
    po, st = CH.compute_case(bad)
    _, poses, got = _result(f, 1)
    f.close()
    assert st["status"] == CH.NOT_POSDEF
    for k in R.STAT_INTS:
        assert got[k] == st[k], (k, got, st)
    for k in R.STAT_DOUBLES:
        assert (np.isnan(got[k]) and np.isnan(st[k])) or R.bits([got[k]])[0] == R.bits([st[k]])[0], (k, got, st)
    np.testing.assert_array_equal(R.bits(poses), R.bits(po))
    np.testing.assert_array_equal(R.bits(poses), R.bits(bad["poses"]))


def test_golden_fixture_on_the_device(gpu):
    cases = CH.load_golden()
    names = list(cases)
    f = _fleet([cases[k][0] for k in names])
    for g, k in enumerate(names):
        _load(f, g, cases[k][0])
    f.poison_scratch(0xFF)
    for g, k in enumerate(names):  # each with its own parameters
        f.compute(g, 1, _params(cases[k][0]["params"]))
    for g, k in enumerate(names):
        R.assert_same_result(*_result(f, g)[1:], cases[k][1], cases[k][2], k)
    f.close()


def test_growing_radius_ring_against_plain_lm(gpu):
    """The independent check: the 64-node ring of radius 9.6 m, on which the PCG mode stops 2e-3 away after all 40
    iterations, held on the device to the plain numpy LM within tests/test_spa_chol_cpu.py's bounds (2.6e-8 in the
    poses, 6.7e-14 relative in the cost; measured on the CPU 8.1e-9 and 5.8e-15)."""
    c = CH.grown_ring(64, 64)
    f = _fleet([c])
    _load(f, 0, c)
    f.compute(0, 1, _params(c["params"]))
    _, poses, st = _result(f, 0)
    f.compute(0, 1, _params(c["params"], "pcg"))  # from the optimum: the PCG mode agrees that it is one
    f.close()
    pp, ps = P.solve(c["poses"], c["ends"], c["means"], c["precs"])
    dev = float(np.abs(poses - pp).max())
    rel = abs(st["final_cost"] - ps["final_cost"]) / ps["final_cost"]
    print(f"grown ring on the device: lm {st['lm_iters']} pose deviation {dev:.3e} relative cost deviation {rel:.3e}")
    assert st["status"] == spa.SPA_OK and st["converged"] == 1 and st["lm_iters"] < 40 and st["cg_iters"] == 0
    assert dev <= 2.6e-8 and rel <= 6.7e-14, (dev, rel)


def test_device_poses_feed_the_grid_rebuild(gpu):
    """spa_device_poses after a direct-mode compute handed straight to kg_build_device (tests/test_spa_gpu.py's
    hand-off, with the other solver)."""
    import torch

    gc = KG.case_cross(S=6, n=67, seed=7)
    rng = np.random.default_rng(21)
    links = [(i, i + 1) for i in range(5)] + [(5, 0), (0, 3), (5, 2)]
    c = R.graph_from_truth(gc["poses"], links, rng, drift=(0.03, 0.03, 0.02))
    po, st = CH.compute_case(c)
    assert st["status"] == CH.OK and st["good_iter"] > 0
    want = KG.create_from_scans(dict(gc, poses=po))
    f = _fleet([c])
    _load(f, 0, c)
    d_ranges = torch.from_numpy(gc["ranges"]).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    f.compute_device(0, 1, _params(c["params"]), hip_stream=s.cuda_stream)
    d_poses, n = f.device_poses(0)
    assert n == 6
    lz = gc["laser"]
    b = karto_grid.OccupancyGridBuilder(
        karto.laser(lz["n_readings"], lz["minimum_angle"], lz["angular_resolution"], lz["minimum_range"],
                    lz["range_threshold"]),
        karto_grid.default_params(lz["maximum_range"], gc["resolution"]), 6, want["width"] * want["height"] + 1000)
    got = b.create_from_scans_device(6, d_ranges, d_poses, hip_stream=s.cuda_stream)
    KG.assert_maps_equal(got, want)
    R.assert_same_result(f.get_nodes(0)[1], f.stats(0), po, st)
    b.close()
    f.close()


def test_solver_and_capacity_arguments(gpu):
    f = SpaFleet(1, 4, 3, 6)
    p = spa.default_params()
    for bad in (7, 2, -1):
        p.solver = bad
        with pytest.raises(spa.Slam2dError):
            f.compute(0, 1, p)
    f.close()
    for blocks in (-1, (1 << 27) + 1):
        with pytest.raises(spa.Slam2dError):
            SpaFleet(1, 4, 3, blocks)
    s = spa.SpaSolver(max_nodes=8, max_constraints=16, solver="cholesky")
    assert s.fleet.max_factor_blocks == 36 and s.params.solver == spa.SPA_SOLVER_CHOLESKY
    truth = R.ring_truth(8)
    c = R.graph_from_truth(truth, R.ring_links(8), np.random.default_rng(9))
    for i, p3 in zip(c["ids"], c["poses"]):
        s.AddNode(int(i), p3)
    for (a, b), z, k in zip(c["ends"], c["means"], c["precs"]):
        assert s.AddConstraint(int(c["ids"][a]), int(c["ids"][b]), z, spa.matrix3_inverse(k.reshape(3, 3))) is True
    corr = s.Compute()
    assert s.stats()["status"] == spa.SPA_OK and s.stats()["converged"] == 1 and s.stats()["cg_iters"] == 0
    got = np.array([p3 for _, p3 in corr])
    assert np.abs(got[:, :2] - truth[:, :2]).max() < 0.05 and np.abs(R.wrap(got[:, 2] - truth[:, 2])).max() < 0.05
    s.close()
    with pytest.raises(ValueError):
        spa.SpaSolver(max_nodes=8, max_constraints=16, params=spa.default_params(), solver="cholesky")
