"""The Karto loop-closure and near-chain candidate search on the GPU (include/slam2d/karto_loop.h) against the CPU
restatement tests/ref/karto_loop_ref.c.  Bar: bit-exact -- every integer of every list and count, every chain field,
the bits of every squared distance and of every reference position.  No tolerance appears anywhere."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "ref"))
import karto_loop_cases as K  # noqa: E402
import karto_loop_ref as R  # noqa: E402

from slam2d import Slam2dError  # noqa: E402
from slam2d import karto_loop as kl  # noqa: E402
from slam2d.karto import KtLaser  # noqa: E402

pytestmark = pytest.mark.gpu


def _laser(d) -> KtLaser:
    return KtLaser(d["minimum_angle"], d["angular_resolution"], d["minimum_range"], d["range_threshold"],
                   d["n_readings"], 0)


def _fleet(case, max_graphs=1, max_scans=None, max_edges=None, max_queries=None) -> kl.LoopSearchFleet:
    """Limits that are no multiple of anything unless given: n + 3 scans, m + 1 edges, queries + 2 slots."""
    n, m, nq = len(case["poses"]), len(case["ends"]), len(case["queries"])
    return kl.LoopSearchFleet(_laser(case["laser"]), kl.default_params(**case["params"]), max_graphs,
                              n + 3 if max_scans is None else max_scans, m + 1 if max_edges is None else max_edges,
                              nq + 2 if max_queries is None else max_queries)


def _load(f, g, case):
    f.set_graph(g, len(case["poses"]), case["ends"])
    f.set_scans(g, 0, case["ranges"], case["poses"])


def _rows(g, queries):
    return [(g, *[int(v) for v in q]) for q in queries]


def _assert_slot(f, slot, want, what):
    got = f.get(slot)
    assert got["status"] == kl.KL_OK, (what, got)
    for k in ("n_near_link", "n_near_loop", "n_loop_chains", "n_near_chains", "loop_index_total", "n_near_long",
              "near_index_total"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert got["n_scans"] == len(want["d2"]), what
    R.assert_same_search(got, want, what)


def _check_case(f, g, case, what):
    ref = R.case_reference(case)
    np.testing.assert_array_equal(R.bits(f.get_reference(g, 0, len(ref))), R.bits(ref), err_msg=what)
    if len(case["queries"]):
        assert f.search(_rows(g, case["queries"])) == len(case["queries"])
        for s, q in enumerate(case["queries"]):
            _assert_slot(f, s, R.search_case(case, q, ref), f"{what} {q.tolist()}")


@pytest.mark.parametrize("name", list(K.directed_cases()))
def test_directed_case(gpu, name):
    case = K.directed_cases()[name]
    f = _fleet(case)
    _load(f, 0, case)
    assert f.counts(0) == (len(case["poses"]), len(case["ends"]))
    _check_case(f, 0, case, name)
    f.close()


def test_poisoned_context(gpu, monkeypatch):
    """SLAM2D_POISON=1: every buffer starts as 0xA5 bytes, so a read of memory the context never wrote shows."""
    monkeypatch.setenv("SLAM2D_POISON", "1")
    for name in ("star", "loop_runs", "near_chains", "circle_scans", "ref65"):
        case = K.directed_cases()[name]
        f = _fleet(case, max_graphs=3)
        _load(f, 1, case)
        _check_case(f, 1, case, f"poisoned {name}")
        # graph 0 is empty: its query is refused in its status, graph 1's still runs
        f.search([(0, 0, 0, -1, -1)] + _rows(1, case["queries"][:1]))
        assert f.result(0)["status"] == kl.KL_EINVAL
        if len(case["queries"]):
            assert f.result(1)["status"] == kl.KL_OK
        f.close()


def test_subrange_refresh_leaves_the_other_scans(gpu):
    case = K.reference_cases()["ref65"]
    f = _fleet(case)
    _load(f, 0, case)
    before = f.get_reference(0)
    moved = dict(case)
    moved["poses"] = case["poses"] + np.array([0.25, -0.5, 0.1])
    f.set_scans(0, 2, case["ranges"][2:5], moved["poses"][2:5])
    after = f.get_reference(0)
    want = R.case_reference(moved)
    np.testing.assert_array_equal(R.bits(after[2:5]), R.bits(want[2:5]))
    np.testing.assert_array_equal(R.bits(after[:2]), R.bits(before[:2]))
    np.testing.assert_array_equal(R.bits(after[5:]), R.bits(before[5:]))
    assert np.any(R.bits(after[2:5]) != R.bits(before[2:5]))
    f.close()


def _shared_params_cases():
    """Graphs of different sizes under one context's parameters."""
    prm = dict(link=0.9, loop=1.8, min_chain=3)
    out = []
    for seed in (11, 12, 13, 14, 15):
        c = K.random_case(seed)
        out.append(K.position_case(c["poses"][:, :2], c["ends"], c["queries"], **prm))
    return out


def test_one_launch_many_graphs_and_prefix_queries(gpu):
    cases = _shared_params_cases()
    sizes = [len(c["poses"]) for c in cases]
    assert len(set(sizes)) == len(sizes)
    big = max(cases, key=lambda c: len(c["poses"]))
    f = _fleet(big, max_graphs=len(cases) + 1, max_edges=max(len(c["ends"]) for c in cases) + 1, max_queries=64)
    for g, c in enumerate(cases):
        _load(f, g, c)
    refs = [f.get_reference(g) for g in range(len(cases))]
    rows, want = [], []
    rng = np.random.default_rng(7)
    for g, c in enumerate(cases[:-1]):  # the last graph takes no part in the launch
        n, m = len(c["poses"]), len(c["ends"])
        qs = [(n - 1, 0, -1, -1), (n // 2, 0, n // 2 + 1, min(m, n // 2)), (0, n // 3, -1, m // 2)]
        qs += [(int(rng.integers(0, k)), int(rng.integers(0, k + 1)), k, int(rng.integers(0, m + 1)))
               for k in rng.integers(1, n + 1, 3)]
        for q in qs:
            rows.append((g, *q))
            want.append(R.search_case(c, np.asarray(q), refs[g]))
    bad = len(rows)
    rows.insert(3, (0, sizes[0], 0, -1, -1))      # scan >= n_scans: refused in its status, the others still run
    want.insert(3, None)
    rows.append((1, 2, 0, 2, -1))                 # scan >= the query's own prefix
    want.append(None)
    rows.append((len(cases) + 5, 0, 0, -1, -1))   # no such graph
    want.append(None)
    assert f.search(rows) == bad + 3
    for s, w in enumerate(want):
        if w is None:
            r = f.result(s)
            assert r["status"] == kl.KL_EINVAL and r["n_loop_chains"] == 0 and r["n_near_chains"] == 0, (s, r)
        else:
            _assert_slot(f, s, w, f"slot {s} {rows[s]}")
    for g, c in enumerate(cases):  # the graphs, the untouched one included, read back unchanged
        assert f.counts(g) == (len(c["poses"]), len(c["ends"]))
        np.testing.assert_array_equal(R.bits(f.get_reference(g)), R.bits(refs[g]))
    # the untouched graph answers afterwards
    last = len(cases) - 1
    f.search(_rows(last, cases[last]["queries"]))
    _assert_slot(f, 0, R.search_case(cases[last], cases[last]["queries"][0], refs[last]), "last graph")
    f.close()


def test_incremental_graph_equals_bulk_and_limits(gpu):
    case = K.case_near_chains()
    n = len(case["poses"])
    f = _fleet(case, max_scans=n, max_edges=len(case["ends"]))
    for k in range(n):
        assert f.add_vertex(0) == k
    with pytest.raises(Slam2dError) as e:
        f.add_vertex(0)
    assert e.value.code == kl.KL_ERANGE and f.counts(0)[0] == n  # refused, not truncated
    for s, t in case["ends"]:
        assert f.add_edge(0, int(s), int(t)) is True
    assert f.add_edge(0, 30, 16) is False and f.add_edge(0, 0, 1) is False  # old: the source's list has that target
    with pytest.raises(Slam2dError) as e:
        f.add_edge(0, 16, 30)  # new (the other direction), but the context is full
    assert e.value.code == kl.KL_ERANGE
    with pytest.raises(Slam2dError) as e:
        f.add_edge(0, 3, 3)
    assert e.value.code == kl.KL_EINVAL
    f.set_scans(0, 0, case["ranges"], case["poses"])
    _check_case(f, 0, case, "incremental")
    # an edit after a search is uploaded before the next one: without the closure edges no near chain is left
    f.set_graph(0, n, case["ends"][:30])
    f.search(_rows(0, case["queries"][:1]))
    cut = dict(case)
    cut["ends"] = case["ends"][:30]
    _assert_slot(f, 0, R.search_case(cut, case["queries"][0]), "after the edit")
    assert f.get(0)["n_near_chains"] == 0
    f.clear_graph(0)
    assert f.counts(0) == (0, 0)
    f.search(_rows(0, case["queries"][:1]))
    assert f.result(0)["status"] == kl.KL_EINVAL
    f.close()
    with pytest.raises(Slam2dError) as e:
        kl.LoopSearchFleet(_laser(case["laser"]), None, 1, kl.KL_MAX_SCANS + 1, 8, 1)
    assert e.value.code == kl.KL_ERANGE


def _spiral(n):
    """n scans 0.05 m apart on a spiral of pitch 0.4 m, every 29th tied to the nearest scan of the ring inside: long
    runs, near-linked lists of several batches that cross rings, every scan in one graph at the scan limit."""
    b = 0.4 / (2.0 * np.pi)
    th = np.sqrt(2.0 * 0.05 * np.arange(1, n + 1) / b)
    xy = np.stack([b * th * np.cos(th), b * th * np.sin(th)], axis=1)
    ends = K.path_edges(n)
    for i in range(150, n, 29):
        j = int(np.argmin(np.sum((xy[:i - 60] - xy[i]) ** 2, axis=1)))
        ends.append((i, j) if i % 2 else (j, i))
    return K.position_case(xy, ends, [(n - 1, 0, -1, -1), (n // 2, 17, -1, -1), (n - 1, 0, n, len(ends) - 5)], link=1.0,
                           loop=2.0, min_chain=5)


@pytest.mark.parametrize("n", [kl.KL_MAX_SCANS, 1000])
def test_graph_at_the_scan_limit(gpu, n):
    case = _spiral(n)
    f = _fleet(case, max_scans=n, max_queries=3)
    _load(f, 0, case)
    _check_case(f, 0, case, f"spiral {n}")
    assert f.get(0)["n_near_link"] > 64 and f.get(0)["n_near_chains"] > 0 and f.get(2)["n_loop_chains"] > 0
    f.close()


def test_device_path_emit_and_closest(gpu):
    """kl_set_scans_device -> kl_search_device -> kl_emit_batch_device on one stream without a host wait, and
    kl_closest_device, against the restatement; the emitted arrays are pool slots in kt_match_batch_device's layout."""
    import torch

    cases = _shared_params_cases()[:3] + [K.position_case(K.case_near_chains()["poses"][:, :2], K.case_near_chains()["ends"],
                                                          K.case_near_chains()["queries"][:1], link=0.9, loop=1.8, min_chain=3)]
    big = max(cases, key=lambda c: len(c["poses"]))
    f = _fleet(big, max_graphs=len(cases), max_edges=max(len(c["ends"]) for c in cases) + 1, max_queries=16)
    offsets = [100, 1000, 5, 40000]
    rows, want, refs, keep_alive = [], [], [], []
    dev = torch.device("cuda")
    for g, c in enumerate(cases):
        f.set_graph(g, len(c["poses"]), c["ends"])
        f.set_pool_offset(g, offsets[g])
        d_r = torch.from_numpy(c["ranges"]).to(dev)
        d_p = torch.from_numpy(c["poses"]).to(dev)
        keep_alive += [d_r, d_p]  # read by the context's stream after this loop moves on
        torch.cuda.synchronize()
        f.set_scans_device(g, 0, len(c["poses"]), d_r.data_ptr(), d_p.data_ptr())
        refs.append(R.case_reference(c))
        n = len(c["poses"])
        for q in [(n - 1, 0, -1, -1), (n // 2, 0, -1, -1), tuple(int(v) for v in c["queries"][0])]:
            rows.append((g, *q))
            want.append(R.search_case(c, np.asarray(q), refs[g]))
    rows.append((0, 10 ** 6, 0, -1, -1))  # refused: emits nothing
    want.append(None)
    d_q = torch.from_numpy(kl.queries(rows).view(np.int32).copy()).to(dev)
    torch.cuda.synchronize()
    f.search_device(len(rows), d_q.data_ptr())
    for which, key, keep in ((kl.KL_LOOP_CHAINS, "loop_chains", lambda ch: True),
                             (kl.KL_NEAR_CHAINS, "near_chains", lambda ch: bool(ch[3] & kl.KL_CHAIN_LONG))):
        exp_q, exp_begin, exp_idx, exp_src = [], [0], [], []
        for s, (row, w) in enumerate(zip(rows, want)):
            if w is None:
                continue
            for ci, ch in enumerate(w[key].tolist()):
                if keep(ch):
                    off = offsets[row[0]]
                    exp_q.append(off + row[1])
                    exp_idx += [off + ch[0] + j for j in range(ch[1])]
                    exp_begin.append(len(exp_idx))
                    exp_src.append([s, ci])
        assert len(exp_q) >= 2, (key, len(exp_q))
        for capacity in (len(exp_q) + 3, len(exp_q), len(exp_q) - 1, 1):
            cap_idx = min(len(rows), capacity) * f.max_scans
            o_q = torch.full((capacity,), -7, dtype=torch.int32, device=dev)
            o_b = torch.full((capacity + 1,), -7, dtype=torch.int32, device=dev)
            o_i = torch.full((cap_idx,), -7, dtype=torch.int32, device=dev)
            o_s = torch.full((capacity, 2), -7, dtype=torch.int32, device=dev)
            o_n = torch.full((1,), -7, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            f.emit_batch_device(len(rows), which, capacity, o_q.data_ptr(), o_b.data_ptr(), o_i.data_ptr(), o_s.data_ptr(),
                                o_n.data_ptr())
            total, status = f.emit_info()
            m = min(capacity, len(exp_q))
            assert int(o_n.cpu()[0]) == m and total == len(exp_q), (key, capacity)
            assert status == (kl.KL_EMIT_OVERFLOW if len(exp_q) > capacity else 0)
            assert o_q.cpu().tolist() == exp_q[:m] + [-7] * (capacity - m)
            assert o_b.cpu().tolist() == exp_begin[:m + 1] + [-7] * (capacity - m)
            assert o_s.cpu().tolist() == exp_src[:m] + [[-7, -7]] * (capacity - m)
            ni = exp_begin[m]
            got_i = o_i.cpu().tolist()
            assert got_i[:ni] == exp_idx[:ni] and all(v == -7 for v in got_i[ni:])
    for s, w in enumerate(want):
        if w is not None:
            _assert_slot(f, s, w, f"device slot {s}")
    # kl_closest_device: chains against the scans' current reference positions
    items, exp = [], []
    for g, c in enumerate(cases):
        n = len(c["poses"])
        for scan, b, ln in [(n - 1, 0, n), (0, n // 2, 1), (n // 3, 1, n - 1), (n - 1, n - 1, 2), (n, 0, 1), (0, -1, 2)]:
            items.append((g, scan, b, ln))
            exp.append(list(R.closest(refs[g], scan, b, ln, 0.9)))
    items.append((99, 0, 0, 1))
    exp.append([-1, 0])
    d_it = torch.tensor(items, dtype=torch.int32, device=dev)
    d_out = torch.full((len(items), 2), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    f.closest_device(len(items), d_it.data_ptr(), d_out.data_ptr())
    f.emit_info()  # waits for the context's last work
    assert d_out.cpu().tolist() == exp
    f.close()


def test_kernel_timing(gpu):
    case = K.case_loop_runs()
    f = _fleet(case)
    f.set_timing(True)
    _load(f, 0, case)
    f.search(_rows(0, case["queries"]))
    t = f.kernel_times(reset=True)
    assert t["kl_reference_kernel"][1] == 1 and t["kl_search_kernel"][1] == 1
    assert t["kl_search_kernel"][0] > 0.0 and t["kl_emit_write_kernel"][1] == 0
    assert f.kernel_times()["kl_search_kernel"][1] == 0
    f.close()
