"""The Karto loop-closure and near-chain candidate search without a GPU: the C restatement the GPU is held to
(tests/ref/karto_loop_ref.c, which uses the run formulations of include/slam2d/karto_loop.h) against the literal
transcription of the reference members (tests/ref/karto_loop_plain.py) and the golden fixture, exactly; hand-derived
results of the directed cases; AddEdge's dedupe rule and the adjacency order of csrc/karto_loop_graph.h through a
stand-alone C++ program under ASan + UBSan; and the barycentre case that separates a sequential from a tree sum."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "ref"))
import karto_loop_cases as K  # noqa: E402
import karto_loop_plain as P  # noqa: E402
import karto_loop_ref as R  # noqa: E402
import make_karto_loop_golden as G  # noqa: E402

from slam2d import karto_loop as kl  # noqa: E402

SWEEP_GRAPHS = 3000


# ------------------------------------------------------------------------------------ 1. restatement == transcription
@pytest.mark.parametrize("name", list(K.search_cases()))
def test_restatement_equals_plain_on_directed_searches(name):
    c = K.search_cases()[name]
    ref = R.case_reference(c)
    for q in c["queries"]:
        R.assert_same_search(R.search_case(c, q, ref), P.search_case(c, q), f"{name} {q.tolist()}")


@pytest.mark.parametrize("name", list(K.reference_cases()))
def test_reference_positions_equal_plain_bit_for_bit(name):
    c = K.reference_cases()[name]
    want = np.array([P.barycenter(c["laser"], c["params"]["use_scan_barycenter"], r, po)
                     for r, po in zip(c["ranges"], c["poses"])])
    got = R.case_reference(c)
    np.testing.assert_array_equal(R.bits(got), R.bits(want))
    # scan 1 has no valid reading: the sensor position
    np.testing.assert_array_equal(R.bits(got[1]), R.bits(c["poses"][1, :2]))
    if not c["params"]["use_scan_barycenter"]:
        np.testing.assert_array_equal(R.bits(got), R.bits(c["poses"][:, :2]))


def test_random_sweep_equals_plain_and_exercises_every_exit():
    """A few thousand graphs of 2 .. 120 scans (random walks and noisy circles, random extra edges, a random query
    index and start_num, every fifth with a prefix): every list identical, every squared distance bit-identical; and
    the sweep meets loop chains, near chains, runs dropped by a near-linked scan and end-of-scans short chains."""
    tot = {k: 0 for k in ("n_loop_chains", "n_near_chains", "dropped_runs", "short_end_chains")}
    for seed in range(SWEEP_GRAPHS):
        c = K.random_case(seed)
        q = c["queries"][0]
        got = R.search_case(c, q)
        R.assert_same_search(got, P.search_case(c, q), f"seed {seed}")
        for k in tot:
            tot[k] += got[k]
    print(tot)
    assert all(v > 0 for v in tot.values()), tot


def test_golden_fixture_reproduces():
    cases = G.load()
    fresh = K.directed_cases()
    assert set(cases) == set(fresh)
    for name, (c, want_ref, want) in cases.items():
        for k in ("ranges", "poses"):
            np.testing.assert_array_equal(R.bits(c[k]), R.bits(fresh[name][k]), err_msg=f"{name} {k}")
        for k in ("ends", "queries"):
            np.testing.assert_array_equal(c[k], fresh[name][k], err_msg=f"{name} {k}")
        assert c["params"] == fresh[name]["params"] and c["laser"] == fresh[name]["laser"], name
        ref = R.case_reference(c)
        np.testing.assert_array_equal(R.bits(ref), R.bits(want_ref), err_msg=name)
        for q, w in zip(c["queries"], want):
            R.assert_same_search(R.search_case(c, q, ref), w, f"{name} {q.tolist()}")


# ------------------------------------------------------------------------------------ 2. hand-derived results
def _one(case, qi=0):
    return R.search_case(case, case["queries"][qi])


def test_threshold_distance_is_in_range_but_not_linked():
    c = K.case_threshold()
    got = _one(c)
    assert got["d2"][3] == 16.0
    assert got["near_link"].tolist() == [0, 1] and got["near_loop"].tolist() == [0, 1]
    assert got["loop_chains"].tolist() == [[2, 2, 4]]  # 2 and 3 are A; the run reaches the end of the scans
    assert _one(c, 1)["loop_chains"].tolist() == [[3, 1, 4]]


def test_traversal_cases():
    got = _one(K.case_through_out_of_range())
    assert got["near_link"].tolist() == [0] and got["near_loop"].tolist() == [0]
    assert got["loop_chains"].tolist() == [[2, 2, 4]]  # 2 and 3 are near, but reachable only through 1
    assert _one(K.case_two_parents())["near_link"].tolist() == [0, 1, 2, 4, 3]
    assert _one(K.case_both_directions())["near_link"].tolist() == [0, 1, 2, 3]
    assert _one(K.case_both_directions(), 1)["near_link"].tolist() == [2, 1, 3, 0]
    star = _one(K.case_star())
    assert star["n_near_link"] == 1 + 100 + 66 and star["near_link"][:4].tolist() == [0, 1, 38, 75]


def test_loop_chain_exits():
    c = K.case_loop_runs()
    want = {0: [[0, 10, 10], [40, 2, 42]], 1: [[40, 2, 42]], 2: [[40, 2, 42]], 3: [[40, 2, 42]], 4: [[41, 1, 42]],
            5: [], 6: [[0, 10, 10]], 7: [[0, 10, 10]]}
    for qi, chains in want.items():
        got = _one(c, qi)
        assert got["loop_chains"].tolist() == chains, qi
        assert got["near_loop"].tolist()[:2] == [36, 35]
    full = _one(c, 0)
    assert full["dropped_runs"] == 1 and full["short_end_chains"] == 1


def test_near_chain_order_filter_and_closest():
    c = K.case_near_chains()
    got = _one(c)
    assert got["near_link"][:5].tolist() == [30, 29, 16, 6, 31]
    # breadth-first order, not index order; the short chain keeps KL_CHAIN_LINKED only; 6 ties with 7 and wins
    assert got["near_chains"].tolist() == [[15, 3, 16, kl.KL_CHAIN_LINKED], [5, 4, 6, kl.KL_CHAIN_LONG | kl.KL_CHAIN_LINKED]]
    assert got["d2"][6] == got["d2"][7]
    assert (got["n_near_long"], got["near_index_total"]) == (1, 4)
    assert _one(c, 3)["near_chains"].tolist() == []  # without the closure edges nothing but the query's run is linked
    assert R.closest(R.case_reference(c), 30, 5, 4, 1.5) == (6, 1)
    assert R.closest(R.case_reference(c), 30, 0, 3, 1.5) == (0, 0)


# ------------------------------------------------------------------------------------ 3. the tree-sum-sensitive scan
def test_tree_sum_differs_from_the_sequential_sum():
    """Scan 5 of the 1081-reading case: the reference's one-at-a-time sum and a pairwise sum differ in at least one bit
    of the barycentre, so the GPU test on this case fails for a kernel that sums by a tree."""
    c = K.reference_cases()["ref1081"]
    seq = R.case_reference(c)
    tree = R.reference(c["laser"], 1, c["ranges"], c["poses"], pairwise=True)
    assert np.any(R.bits(seq[5]) != R.bits(tree[5]))
    np.testing.assert_allclose(seq, tree, rtol=1e-12, atol=1e-12)  # the same sum up to rounding
    np.testing.assert_array_equal(R.bits(seq[6]), R.bits(tree[6]))  # one valid reading: nothing to reorder


# ------------------------------------------------------------------------------------ 4. the host graph
@pytest.fixture(scope="module")
def graph_check(tmp_path_factory):
    """tests/cpp/karto_loop_graph_check.cpp under ASan + UBSan; a stand-alone program."""
    exe = str(tmp_path_factory.mktemp("kl_graph") / "karto_loop_graph_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan",
                    "-static-libubsan", "-fno-sanitize-recover=all", "-I", R.CSRC,
                    os.path.join(HERE, "cpp", "karto_loop_graph_check.cpp"), "-o", exe], check=True)

    def run(n, calls):
        line = " ".join(str(v) for v in [n, len(calls)] + [e for st in calls for e in st]) + "\n"
        r = subprocess.run([exe], input=line, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        return json.loads(r.stdout)

    return run


def test_add_edge_dedupe_and_adjacency_order(graph_check):
    # a -> b twice: old; b -> a: new (the lookup runs over the source's list for the TARGET); then a -> b again: old
    out = graph_check(4, [(0, 1), (0, 1), (1, 0), (0, 1), (1, 0), (2, 1), (1, 2), (3, 0), (0, 3)])
    assert out["ok"] == 1
    assert out["is_new"] == [1, 0, 1, 0, 0, 1, 1, 1, 1]
    assert out["ends"] == [[0, 1], [1, 0], [2, 1], [1, 2], [3, 0], [0, 3]]
    assert out["adj_off"] == [0, 4, 8, 10, 12]
    assert out["adj"][:4] == [[1, 0], [1, 1], [3, 4], [3, 5]]  # vertex 0: its edges in insertion order
    off, adj = R.build_adj(4, out["ends"])  # the tests' own adjacency builder agrees
    assert off.tolist() == out["adj_off"] and adj.tolist() == out["adj"]
    rng = np.random.default_rng(4)
    for n in (2, 7, 40):
        calls = [tuple(int(v) for v in rng.choice(n, 2, replace=False)) for _ in range(6 * n)]
        out = graph_check(n, calls)
        assert out["ok"] == 1 and 0 < sum(out["is_new"]) <= len(calls)
        off, adj = R.build_adj(n, out["ends"])
        assert off.tolist() == out["adj_off"] and adj.tolist() == out["adj"]
        g = P.Graph()
        for _ in range(n):
            g.add_vertex()
        assert [int(g.add_edge(s, t)[1]) for s, t in calls] == out["is_new"]  # the transcription's AddEdge
        assert [[a.obj for a in v.adjacent()] for v in g.vertices] == \
            [[x[0] for x in out["adj"][out["adj_off"][v]:out["adj_off"][v + 1]]] for v in range(n)]


# ------------------------------------------------------------------------------------ 5. the public interface
def test_params_and_layouts():
    d, n = kl.default_params(), kl.node_params()
    assert (d.link_scan_maximum_distance, d.loop_search_maximum_distance, d.loop_match_minimum_chain_size,
            d.use_scan_barycenter) == (10.0, 4.0, 10, 1)
    assert (n.link_scan_maximum_distance, n.loop_search_maximum_distance, n.loop_match_minimum_chain_size,
            n.use_scan_barycenter) == (1.5, 10.0, 5, 1)
    assert ctypes.sizeof(kl.KlParams) == 24 and ctypes.sizeof(kl.KlResult) == 40 == kl.RESULT_DTYPE.itemsize
    assert kl.QUERY_DTYPE.itemsize == 20 and kl.LOOP_CHAIN_DTYPE.itemsize == 16 == kl.NEAR_CHAIN_DTYPE.itemsize
    L = kl._lib.lib()
    assert L.kl_version().decode().startswith("slam2d-karto-loop")
    names = [L.kl_kernel_name(i).decode() for i in range(L.kl_num_kernels())]
    assert names[:2] == ["kl_reference_kernel", "kl_search_kernel"] and len(set(names)) == len(names)
    # the header's constants are the module's
    hdr = open(os.path.join(REPO, "include", "slam2d", "karto_loop.h")).read()
    for k in ("KL_MAX_SCANS", "KL_NEAR_CHAINS", "KL_CHAIN_LONG", "KL_CHAIN_LINKED", "KL_EMIT_OVERFLOW"):
        assert f"#define {k} {getattr(kl, k)}" in hdr, k
    assert "#define KL_ERANGE (-5)" in hdr and kl.KL_ERANGE == -5
