"""GPU parity of the pose-graph optimiser (SysSPA2d::doSPA in its block-Jacobi PCG mode, spa_solve_kernel) against
the CPU restatement tests/ref/spa2d_ref.c.  Bar: bit-exact -- every pose's bits, the bits of the initial and final
cost and of lambda, every integer of the stats.  The restatement scatters as the reference does and the kernel
gathers, so the gather orders are under test.  The context's scratch is poisoned before each launch, and graphs
outside the computed range are read back unchanged.  Eigen and SuiteSparse are absent: parity with the compiled
library is unpinned.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import karto_grid_ref as KG  # noqa: E402
import spa2d_ref as R  # noqa: E402

from slam2d import karto, karto_grid, spa  # noqa: E402
from slam2d.spa import SpaFleet  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {
    # node counts 2, 3, 4
    "tiny2": lambda: R.case_tiny(2), "tiny3": lambda: R.case_tiny(3), "tiny4": lambda: R.case_tiny(4),
    # free-node counts at the reduction's fold boundaries; the chains also give 256 and 257 constraints
    "free255": lambda: R.case_ring(256, 31), "free256_cons256": lambda: R.case_chain(257, 32),
    "free257_cons257": lambda: R.case_chain(258, 33), "free513": lambda: R.case_ring(514, 34),
    "hub": R.case_hub, "reversed": R.case_reversed, "repeated": R.case_repeated, "near_pi": R.case_near_pi,
    "fixed2": lambda: R.case_ring(12, 4, n_fixed=2),
    "reject1": lambda: R.case_outliers(R.REJECT_ONCE_SEED), "reject2": lambda: R.case_outliers(R.REJECT_TWICE_SEED),
    "cg2": lambda: R.case_ring(33, 5, max_cg_iters=2), "niter3": lambda: R.case_ring(33, 6, niter=3),
    "tol2": lambda: R.case_ring(12, 7, init_tol=2.0), "abstol": lambda: R.case_ring(12, 2),
}


@functools.lru_cache(maxsize=None)
def _want(name):
    """A named case and the restatement's result, computed once and shared (treat as read-only)."""
    c = CASES[name]()
    po, st = R.compute_case(c)
    return c, po, st


def _params(prm: dict) -> spa.SpaParams:
    return spa.default_params(**prm)


def _fleet(cases, extra=0) -> SpaFleet:
    n = max(len(c["poses"]) for c in cases)
    m = max(len(c["ends"]) for c in cases)
    return SpaFleet(len(cases) + extra, n + 3, m + 5)  # limits that are no multiple of anything


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
    f.poison_scratch(0xFF)  # NaN doubles: a value read before it is written spreads
    f.compute(0, 1, _params(c["params"]))
    ids, poses, st = _result(f, 0)
    np.testing.assert_array_equal(ids, c["ids"])
    R.assert_same_result(poses, st, want_poses, want_stats, name)
    f.close()


def test_the_cases_take_the_paths_they_are_named_for(gpu):
    """What the restatement's stats say about the cases above (the GPU equals them bit for bit)."""
    assert _want("reject1")[2]["rejected"] == 1 and _want("reject2")[2]["rejected"] == 2
    assert _want("niter3")[2]["lm_iters"] == 3 and _want("niter3")[2]["converged"] == 0
    assert _want("tol2")[2]["cg_iters"] == 0 and _want("tol2")[2]["converged"] == 1
    assert _want("abstol")[2]["abstol_hits"] > 0
    assert 40 < _want("cg2")[2]["cg_iters"] <= 80
    for name, free, cons in (("free255", 255, None), ("free256_cons256", 256, 256), ("free257_cons257", 257, 257),
                             ("free513", 513, None), ("tiny2", 1, 1)):
        c = _want(name)[0]
        assert len(c["poses"]) - c["params"]["n_fixed"] == free and (cons is None or len(c["ends"]) == cons)
    c = _want("hub")[0]
    nb = {int(b if a == 45 else a) for a, b in c["ends"] if 45 in (a, b)}
    assert len(nb) == 40 and sum(v < 45 for v in nb) == 20
    assert all(a > b for a, b in _want("reversed")[0]["ends"])
    c, po, _ = _want("near_pi")
    assert np.all(np.abs(np.abs(c["poses"][:, 2]) - np.pi) < 1e-1) and np.any(np.sign(po[:, 2]) != np.sign(c["poses"][:, 2]))


def test_fleet_of_five_in_one_launch(gpu):
    """Five sizes in one launch, an empty graph, a disconnected one and one without a fixed node among them: the
    others still run, and each graph's bits equal its solo run."""
    cases = [_want("abstol")[0], R.case_empty(), R.case_disconnected(), R.case_ring(33, 3), _want("hub")[0]]
    n_fixed = [None, None, None, 0, None]
    f = _fleet(cases)
    for g, (c, nf) in enumerate(zip(cases, n_fixed)):
        _load(f, g, c)
        f.set_n_fixed(g, nf)
    f.poison_scratch(0xFF)
    f.compute(0, 5, _params(R.DEFAULTS))
    got = [_result(f, g) for g in range(5)]
    f.close()
    assert [s["status"] for _, _, s in got] == [spa.SPA_OK, spa.SPA_OK, spa.SPA_DISCONNECTED, spa.SPA_NO_FIXED, spa.SPA_OK]
    for g, (c, nf) in enumerate(zip(cases, n_fixed)):
        po, st = R.compute_case(c, **({} if nf is None else {"n_fixed": nf}))
        R.assert_same_result(got[g][1], got[g][2], po, st, f"graph {g}")
        solo = _fleet([c])
        _load(solo, 0, c)
        solo.set_n_fixed(0, nf)
        solo.compute(0, 1, _params(R.DEFAULTS))
        _, sp, ss = _result(solo, 0)
        solo.close()
        R.assert_same_result(got[g][1], got[g][2], sp, ss, f"graph {g} solo")
    for g in (2, 3):  # refused graphs keep their poses
        np.testing.assert_array_equal(R.bits(got[g][1]), R.bits(cases[g]["poses"]))


def test_graphs_outside_the_range_are_untouched(gpu):
    cs = [_want("tiny3")[0], _want("abstol")[0], _want("fixed2")[0], _want("tiny4")[0]]
    f = _fleet(cs)
    for g, c in enumerate(cs):
        _load(f, g, c)
    f.poison_scratch(0xFF)
    f.compute(1, 2, _params(R.DEFAULTS))
    for g in (0, 3):
        _, poses, st = _result(f, g)
        np.testing.assert_array_equal(R.bits(poses), R.bits(cs[g]["poses"]))
        assert st["status"] == spa.SPA_NOT_RUN
    R.assert_same_result(*_result(f, 1)[1:], *_want("abstol")[1:], "graph 1")
    po, st = R.compute_case(cs[2], n_fixed=1)  # the launch's params, not the case's
    R.assert_same_result(*_result(f, 2)[1:], po, st, "graph 2")
    f.close()


def test_compute_grow_compute(gpu):
    """Poses persist in the context: compute, add nodes and constraints by id, compute again, against the
    restatement doing the same.  The ids include a duplicate (the last wins) and an unknown one (nothing added)."""
    c = _want("abstol")[0]
    f = SpaFleet(1, 40, 90)
    ref = R.RefGraph()
    for i, p in zip(c["ids"], c["poses"]):
        f.add_node(0, int(i), p)
        ref.add_node(int(i), p)
    for (a, b), z, k in zip(c["ends"], c["means"], c["precs"]):
        assert f.add_constraint(0, int(c["ids"][a]), int(c["ids"][b]), z, k) is True
        assert ref.add_constraint(int(c["ids"][a]), int(c["ids"][b]), z, k) is True
    prm = _params(R.DEFAULTS)
    f.poison_scratch(0xFF)
    f.compute(0, 1, prm)
    st = ref.compute()
    _, poses, got = _result(f, 0)
    R.assert_same_result(poses, got, np.asarray(ref.poses), st, "first")
    R.assert_same_result(poses, got, *_want("abstol")[1:], "first, bulk form")
    rng = np.random.default_rng(5)
    last = int(c["ids"][-1])
    new = [(500, [0.3, 2.1, 3.0]), (501, [-0.4, 2.0, -2.9]), (500, [-0.9, 1.7, -2.6])]  # id 500 twice
    for i, p in new:
        f.add_node(0, i, p)
        ref.add_node(i, p)
    for id0, id1 in [(last, 500), (500, 501), (501, 500), (100, 501), (999, 500), (500, 999)]:
        z, k = rng.normal(0.0, 0.3, 3), R.random_prec(rng)
        a, b = f.add_constraint(0, id0, id1, z, k), ref.add_constraint(id0, id1, z, k)
        assert a == b == (999 not in (id0, id1))
    assert f.counts(0) == (len(ref.ids), len(ref.ends))
    before = np.asarray(ref.poses).copy()
    _, poses, _ = _result(f, 0)  # optimised poses from the device, the new nodes' from the host
    np.testing.assert_array_equal(R.bits(poses), R.bits(before))
    # node index 12 (the first id 500) has no constraint: the last node with the id took them all
    f.poison_scratch(0xFF)
    f.compute(0, 1, prm)
    st = ref.compute()
    assert st["status"] == R.DISCONNECTED
    _, poses, got = _result(f, 0)
    R.assert_same_result(poses, got, np.asarray(ref.poses), st, "disconnected")
    z, k = rng.normal(0.0, 0.3, 3), R.random_prec(rng)
    f.set_n_fixed(0, 1)
    ends_before = len(ref.ends)
    ref.ends.append([12, 3])  # by index: ids cannot name the shadowed node
    ref.means.append(z.tolist())
    ref.precs.append(k.tolist())
    f.set_graph(0, ref.ids, before, ref.ends, ref.means, ref.precs)  # the bulk form, same poses
    assert f.counts(0)[1] == ends_before + 1
    f.poison_scratch(0xFF)
    f.compute(0, 1, prm)
    st = ref.compute()
    assert st["status"] == R.OK and st["good_iter"] > 0
    _, poses, got = _result(f, 0)
    R.assert_same_result(poses, got, np.asarray(ref.poses), st, "second")
    f.close()


def test_host_and_device_entry_points_agree(gpu):
    import torch

    c, want_poses, want_stats = _want("reversed")
    f = _fleet([c], extra=1)
    _load(f, 0, c)
    _load(f, 1, c)
    prm = _params(c["params"])
    f.compute(0, 1, prm)
    s = torch.cuda.Stream()
    f.compute_device(1, 1, prm, hip_stream=s.cuda_stream)
    ptr, n = f.device_poses(1)
    assert n == len(c["poses"]) and ptr
    s.synchronize()
    for g in (0, 1):
        _, poses, st = _result(f, g)
        R.assert_same_result(poses, st, want_poses, want_stats, f"graph {g}")
    f.close()


def test_argument_errors(gpu):
    f = SpaFleet(2, 4, 3)
    L, h = f.L, f.h
    for i in range(4):
        f.add_node(0, i, [float(i), 0.0, 0.0])
    assert L.spa_add_node(h, 0, 9, np.zeros(3).ctypes.data) == spa.SPA_ERANGE
    with pytest.raises(spa.Slam2dError):
        f.add_constraint(0, 1, 1, [0, 0, 0], np.eye(3))  # a node to itself
    with pytest.raises(spa.Slam2dError):
        f.add_node(2, 0, [0, 0, 0])  # no such graph
    for kw in ({"niter": -1}, {"niter": 1001}, {"max_cg_iters": 65537}, {"niter": 1000, "max_cg_iters": 2000},
               {"lambda": 0.0}, {"init_tol": float("nan")}):
        with pytest.raises(spa.Slam2dError):
            f.compute(0, 1, spa.default_params(**kw))
    with pytest.raises(spa.Slam2dError):
        f.compute(1, 2)
    p = spa.default_params()
    assert (p.niter, p.max_cg_iters, p.n_fixed, p.lambda_, p.init_tol) == (40, 50, 1, 1e-4, 1e-8)
    f.close()


def test_spa_solver_mirror(gpu):
    """SpaSolver's reference method names over one graph: AddNode / AddConstraint / Compute / GetCorrections /
    Clear, with LinkInfo's pose difference and covariance feeding AddConstraint as spa_solver.cc:77-90 does."""
    truth = R.ring_truth(8)
    rng = np.random.default_rng(9)
    s = spa.SpaSolver(max_nodes=8, max_constraints=16)
    ref = R.RefGraph()
    pose = truth[0].copy()
    for i in range(8):
        if i:
            pose = R.compose(pose, R.relative(truth[i - 1], truth[i]) + rng.normal(0.0, 0.02, 3))
        s.AddNode(10 + i, pose)
        ref.add_node(10 + i, pose)
    cov = np.diag([0.01, 0.02, 0.005])
    for a, b in R.ring_links(8, two_hop=False):
        mean, cv = spa.link_info(truth[a], truth[b], cov)
        assert s.AddConstraint(10 + a, 10 + b, mean, cv) is True
        assert ref.add_constraint(10 + a, 10 + b, mean, spa.precision_of(cv)) is True
    assert s.AddConstraint(10, 99, mean, cv) is False
    corr = s.Compute()
    st = ref.compute()
    assert corr is s.GetCorrections() and [i for i, _ in corr] == ref.ids
    R.assert_same_result(np.array([p for _, p in corr]), s.stats(), np.asarray(ref.poses), st)
    assert np.abs(np.array([p for _, p in corr]) - truth).max() < 0.05  # the drift is gone
    s.Clear()
    assert s.GetCorrections() == []
    assert [i for i, _ in s.Compute()] == ref.ids  # Clear keeps the graph (spa_solver.cc:32-35)
    s.close()


def test_device_poses_feed_the_grid_rebuild(gpu):
    """spa_device_poses handed straight to kg_build_device: the planes equal the restatement's grid of the
    restatement's poses (the `mini` grid case's laser and ranges, its six poses as a drifted chain with a closure)."""
    import torch

    gc = KG.case_cross(S=6, n=67, seed=7)
    truth = gc["poses"]
    rng = np.random.default_rng(21)
    links = [(i, i + 1) for i in range(5)] + [(5, 0), (0, 3)]
    c = R.graph_from_truth(truth, links, rng, drift=(0.03, 0.03, 0.02))
    po, st = R.compute_case(c)
    assert st["status"] == R.OK and st["good_iter"] > 0
    want = KG.create_from_scans(dict(gc, poses=po))
    f = _fleet([c])
    _load(f, 0, c)
    d_ranges = torch.from_numpy(gc["ranges"]).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()  # one stream for both calls: the rebuild is ordered after the compute, no host wait between
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
