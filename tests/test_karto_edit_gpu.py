"""GPU parity of the Karto graph edits on the device (kl_edit_*_device, spa_edit_*_device, kd_commit_*_device) against
the host path of the same library: every test runs a device-edited fleet beside a host-edited twin (kl_add_vertex,
kl_add_edge, spa_add_node, spa_add_constraint, then the upload) and compares the contexts' device arrays, read back
through kl_download_graph / spa_download_graph, bit for bit.  Directed cases are also held to the transcription's graph
(tests/ref/karto_loop_plain.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "ref"))
sys.path.insert(0, HERE)
import karto_loop_plain as LP  # noqa: E402

from slam2d import karto_edit as kd  # noqa: E402
from slam2d import karto_link as ke  # noqa: E402
from slam2d import karto_loop as kl  # noqa: E402
from slam2d import karto_process as kp  # noqa: E402
from slam2d import spa as sp  # noqa: E402
from slam2d.karto import KtLaser  # noqa: E402

pytestmark = pytest.mark.gpu

KL_PRM = dict(link_scan_maximum_distance=1.5, loop_search_maximum_distance=4.0, loop_match_minimum_chain_size=3,
              use_scan_barycenter=0)
PREC = np.array([[120.0, 3.0, -2.0], [3.0, 90.0, 1.5], [-2.0, 1.5, 400.0]])


def laser():
    return KtLaser(-1.0, 0.25, 0.1, 4.0, 8, 0)


def dev(a):
    """The bytes of a host array on the device (spare bytes, so that an empty array still has an address)."""
    import torch

    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([b, np.zeros(16, np.uint8)])).cuda()


def host(t, dtype, n):
    return t.cpu().numpy()[:n * np.dtype(dtype).itemsize].copy().view(dtype)


def blank(n):
    return dev(np.full(max(n, 1), -77, np.int32))


def same(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {k}\n{x}\n{y}"
        else:
            assert x == y, f"{what}: {k} {x} {y}"


class Twin:
    """A device-edited LoopSearchFleet + SpaFleet beside a host-edited pair; every edit goes to both, the host pair by
    the host entry points with the refusals the device rows get."""

    def __init__(self, G, N, M, spa_nodes=None, spa_cons=None, factor=0, with_spa=True):
        mk = lambda: kl.LoopSearchFleet(laser(), kl.default_params(**KL_PRM), G, N, M, G)  # noqa: E731
        self.G, self.N = G, N
        self.fd, self.fh = mk(), mk()
        self.sd = self.sh = None
        if with_spa:
            self.sd = sp.SpaFleet(G, spa_nodes or N, spa_cons or M, factor)
            self.sh = sp.SpaFleet(G, spa_nodes or N, spa_cons or M, factor)
        self.L = self.fd.L
        self.seen = dict(old=0, new=0, refused=0)

    def close(self):
        for c in (self.fd, self.fh, self.sd, self.sh):
            if c is not None:
                c.close()

    # ---------------------------------------------------------------- kl
    def vertices(self, rows, enqueue_only=False):
        """rows of (graph, expected id or -1)."""
        r = np.asarray(rows, np.int32).reshape(-1, 2)
        n = len(r)
        d_g, d_e, d_id, d_st = dev(r[:, 0].copy()), dev(r[:, 1].copy()), blank(n), blank(n)
        self.fd.edit_vertices_device(n, d_g.data_ptr(), d_e.data_ptr(), d_id.data_ptr(), d_st.data_ptr())
        want_id, want_st = [], []
        for g, ex in r.tolist():
            if g < 0:
                want_id.append(-1), want_st.append(0)
                continue
            cnt = self.fh.counts(g)[0]
            if ex >= 0 and ex != cnt:
                want_id.append(-1), want_st.append(kl.KL_EINVAL)
                continue
            sid = ctypes.c_int(-1)
            rc = self.L.kl_add_vertex(self.fh.h, g, ctypes.byref(sid))
            want_id.append(sid.value if rc == 0 else -1), want_st.append(rc)
        self.seen["refused"] += sum(s != 0 for s in want_st)
        self._keep = (d_g, d_e, d_id, d_st)
        if enqueue_only:
            return lambda: self._check_out(d_id, d_st, want_id, want_st, n, "vertex")
        self._check_out(d_id, d_st, want_id, want_st, n, "vertex")
        return want_id, want_st

    def _check_out(self, d_val, d_st, want_val, want_st, n, what):
        assert host(d_val, np.int32, n).tolist() == want_val, f"{what} values"
        assert host(d_st, np.int32, n).tolist() == want_st, f"{what} status"

    def edges(self, rows, enqueue_only=False):
        """rows of (graph, source, target)."""
        r = np.zeros(len(rows), kl.EDGE_ROW_DTYPE)
        for i, (g, s, t) in enumerate(rows):
            r[i] = (g, s, t, 0)
        n = len(r)
        d_r, d_new, d_st = dev(r), blank(n), blank(n)
        self.fd.edit_edges_device(n, d_r.data_ptr(), d_new.data_ptr(), d_st.data_ptr())
        want_new, want_st = [], []
        for g, s, t in rows:
            if g < 0:
                want_new.append(0), want_st.append(0)
                continue
            nw = ctypes.c_int(0)
            want_st.append(self.L.kl_add_edge(self.fh.h, g, s, t, ctypes.byref(nw)))
            want_new.append(nw.value)
        self.seen["refused"] += sum(s != 0 for s in want_st)
        self.seen["new"] += sum(want_new)
        self.seen["old"] += sum(1 for (g, _, _), s, w in zip(rows, want_st, want_new) if g >= 0 and s == 0 and not w)
        self._keep2 = (d_r, d_new, d_st)
        if enqueue_only:
            return want_new, d_new, lambda: self._check_out(d_new, d_st, want_new, want_st, n, "edge")
        self._check_out(d_new, d_st, want_new, want_st, n, "edge")
        return want_new, d_new, want_st

    # ---------------------------------------------------------------- spa
    def nodes(self, rows, mask=None):
        """rows of (graph, id, pose[3]); mask a list of ints or None."""
        r = np.zeros(len(rows), sp.NODE_ROW_DTYPE)
        for i, (g, id_, pose) in enumerate(rows):
            r[i] = (g, id_, pose)
        n = len(r)
        d_r, d_st = dev(r), blank(n)
        d_m = dev(np.asarray(mask, np.int32)) if mask is not None else None
        self.sd.edit_nodes_device(n, d_r.data_ptr(), d_m.data_ptr() if d_m is not None else 0, d_st.data_ptr())
        want = []
        for i, (g, id_, pose) in enumerate(rows):
            if g < 0 or (mask is not None and mask[i] != 1):
                want.append(0)
                continue
            p = np.ascontiguousarray(pose, np.float64)
            want.append(self.L.spa_add_node(self.sh.h, g, id_, p.ctypes.data_as(ctypes.c_void_p)))
        assert host(d_st, np.int32, n).tolist() == want, "node status"
        self.seen["refused"] += sum(s != 0 for s in want)
        return want

    def cons(self, rows, mask=None, d_mask=None):
        """rows of (graph, id0, id1, mean[3], prec[9]); the mask as host ints (applied to the twin) and, when it is
        already on the device, its tensor."""
        r = np.zeros(len(rows), sp.CON_ROW_DTYPE)
        for i, (g, a, b, mean, prec) in enumerate(rows):
            r[i] = (g, a, b, 0, mean, np.asarray(prec).reshape(9))
        n = len(r)
        d_r, d_add, d_st = dev(r), blank(n), blank(n)
        if d_mask is None and mask is not None:
            d_mask = dev(np.asarray(mask, np.int32))
        self.sd.edit_constraints_device(n, d_r.data_ptr(), d_mask.data_ptr() if d_mask is not None else 0, d_add.data_ptr(),
                                        d_st.data_ptr())
        want_add, want_st = [], []
        for i, (g, a, b, mean, prec) in enumerate(rows):
            if g < 0 or (mask is not None and mask[i] != 1):
                want_add.append(0), want_st.append(0)
                continue
            m_, k_ = np.ascontiguousarray(mean, np.float64), np.ascontiguousarray(prec, np.float64).reshape(9)
            added = ctypes.c_int(0)
            want_st.append(self.L.spa_add_constraint(self.sh.h, g, a, b, m_.ctypes.data_as(ctypes.c_void_p),
                                                     k_.ctypes.data_as(ctypes.c_void_p), ctypes.byref(added)))
            want_add.append(added.value)
        assert host(d_add, np.int32, n).tolist() == want_add, "constraint added"
        assert host(d_st, np.int32, n).tolist() == want_st, "constraint status"
        self.seen["refused"] += sum(s != 0 for s in want_st)
        return want_add, want_st

    # ---------------------------------------------------------------- comparison
    def compare(self, what=""):
        for g in range(self.G):
            same(self.fd.download_graph(g), self.fh.download_graph(g), f"{what} kl graph {g}")
            if self.sd is not None:
                same(self.sd.download_graph(g), self.sh.download_graph(g), f"{what} spa graph {g}")

    def compare_compute(self, solver, what=""):
        p = sp.default_params(solver=solver, niter=8)
        self.sd.compute(0, self.G, p)
        self.sh.compute(0, self.G, p)
        for g in range(self.G):
            a, b = self.sd.get_nodes(g), self.sh.get_nodes(g)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), f"{what} {solver} poses of graph {g}"
            sa, sb = self.sd.stats(g), self.sh.stats(g)
            assert repr(sa) == repr(sb), f"{what} {solver} stats of graph {g}: {sa} {sb}"


def plain_graph(n, calls):
    g = LP.Graph()
    for _ in range(n):
        g.add_vertex()
    is_new = [int(g.add_edge(s, t)[1]) for s, t in calls]
    adj = [[(a.obj) for a in v.adjacent()] for v in g.vertices]
    return is_new, adj


def adjacency(d):
    return [d["adj"][d["adj_off"][v]:d["adj_off"][v + 1], 0].tolist() for v in range(d["n_scans"])]


# ------------------------------------------------------------------------------------ 1. kl directed
DIRECTED = [(0, 1), (0, 1), (1, 0), (2, 2), (1, 5), (3, 4), (0, 1), (1, 0)]  # graph 0 and, shifted, graph 1; 5 vertices


@pytest.mark.parametrize("calls", [1, 2])
def test_kl_directed_rows_of_two_graphs_interleaved(gpu, calls):
    tw = Twin(3, 8, 16, with_spa=False)
    ids, st = tw.vertices([(g, -1) for _ in range(5) for g in (0, 1)] + [(-1, -1), (2, 3), (2, 0), (2, 0)])
    assert ids[-4:] == [-1, -1, 0, -1] and st[-4:] == [0, kl.KL_EINVAL, 0, kl.KL_EINVAL]  # the expected-id rule
    rows = []
    for i, (s, t) in enumerate(DIRECTED):
        rows += [(0, s, t), (1, t, s)]
        if i == 2:
            rows.append((-1, 0, 1))  # a skipped row
    cut = len(rows) if calls == 1 else 7
    got_new, got_st = [], []
    for part in (rows[:cut], rows[cut:]):
        if part:
            w, _, s_ = tw.edges(part)
            got_new += w
            got_st += s_
    tw.compare(f"{calls} call(s)")
    for g in (0, 1):
        mine = [(s, t) if g == 0 else (t, s) for s, t in DIRECTED]
        legal = [(s, t) for s, t in mine if s != t and max(s, t) < 5]
        is_new, adj = plain_graph(5, legal)
        it = iter(is_new)
        want = [next(it) if (s != t and max(s, t) < 5) else 0 for s, t in mine]
        got = [w for (gg, _, _), w in zip(rows, got_new) if gg == g]
        assert got == want and want == [1, 0, 1, 0, 0, 1, 0, 0], (g, got, want)
        assert adjacency(tw.fd.download_graph(g)) == adj
    bad = [s_ for (gg, _, _), s_ in zip(rows, got_st) if gg == 0]
    assert bad == [0, 0, 0, kl.KL_EINVAL, kl.KL_EINVAL, 0, 0, 0]  # the self edge, the end equal to n_scans
    n_ref, first = tw.fd.edit_info()
    assert (n_ref, first) == (2 + 4, kl.KL_EINVAL)
    assert tw.fd.edit_info() == (0, 0)
    tw.close()


def test_kl_star_isolated_vertex_and_full_graph(gpu):
    tw = Twin(3, 80, 74, with_spa=False)
    tw.vertices([(0, -1)] * 72 + [(1, -1)] * 3 + [(2, -1)] * 2)
    # a hub with 70 edges, then duplicates of its 1st, 64th, 65th and 70th: the lookup over the hub's list passes one
    # wave's width
    star = [(0, 0, k) for k in range(1, 71)]
    new, _, st = tw.edges(star)
    assert new == [1] * 70 and not any(st)
    dup = [star[0], star[63], star[64], star[69]]
    new, _, st = tw.edges([(2, 0, 1)] + dup + [(0, 71, 70)])
    assert new == [1, 0, 0, 0, 0, 1] and not any(st)
    tw.compare("star")
    d = tw.fd.download_graph(0)
    assert d["adj_off"][1] == 70 and adjacency(d)[0] == list(range(1, 71))
    # graph 1: a vertex with no edge between two that have some
    tw.edges([(1, 0, 2), (1, 2, 0)])
    assert adjacency(tw.fd.download_graph(1)) == [[2, 2], [], [0, 0]]
    tw.compare("isolated")
    # fill graph 0 to exactly max_scans and max_edges; one more of each is refused, the next graph's row applied
    tw.vertices([(0, -1)] * (80 - 72))
    have = tw.fd.download_graph(0)["n_edges"]
    tw.edges([(0, 72 + k % 8, k % 60 + 1) for k in range(74 - have)])
    assert tw.fd.counts(0) == (80, 74)
    ids, st = tw.vertices([(0, -1), (2, -1)])
    assert ids == [-1, 2] and st == [kl.KL_ERANGE, 0]
    new, _, st = tw.edges([(0, 79, 78), (2, 2, 0), (0, 0, 1)])
    assert new == [0, 1, 0] and st == [kl.KL_ERANGE, 0, 0]  # a full graph still answers "old" for an edge it has
    tw.compare("full")
    assert tw.fd.edit_info() == (2, kl.KL_ERANGE)
    tw.close()


# ------------------------------------------------------------------------------------ 2. spa directed
def ring(g, n, m, rng, id_of=lambda k: k):
    """n nodes and m constraints of graph g: a chain first, then random pairs."""
    nodes = [(g, id_of(k), rng.normal(size=3) * [1.0, 1.0, 0.1] + [0.4 * k, 0.0, 0.0]) for k in range(n)]
    cons = []
    for c in range(m):
        a = c if c < n - 1 else int(rng.integers(0, n))
        b = a + 1 if c < n - 1 else int((a + 1 + rng.integers(0, n - 1)) % n)
        cons.append((g, id_of(a), id_of(b), rng.normal(size=3) * 0.3 + [0.4, 0, 0], PREC + rng.uniform(0, 1) * np.eye(3)))
    return nodes, cons


def test_spa_directed(gpu):
    rng = np.random.default_rng(7)
    sizes = [(1, 0), (2, 1), (63, 64), (64, 65), (65, 300), (257, 300)]
    N, M = 257, 300
    tw = Twin(len(sizes) + 1, 4, 4, spa_nodes=N, spa_cons=M, factor=N * (N + 1) // 2)
    all_nodes, all_cons = [], []
    for g, (n, m) in enumerate(sizes):
        nodes, cons = ring(g, n, m, rng, id_of=lambda k: 1000 - 3 * k)
        all_nodes.append(nodes), all_cons.append(cons)
    # the nodes of all graphs interleaved, one row masked out, one skipped
    inter = [all_nodes[g][k] for k in range(N) for g in range(len(sizes)) if k < sizes[g][0]]
    inter.insert(5, (-1, 0, np.zeros(3)))
    mask = [1] * len(inter)
    mask[9] = 0
    again = inter[9]
    tw.nodes(inter, mask)
    tw.nodes([again])
    tw.compare("nodes")
    inter = [all_cons[g][c] for c in range(M) for g in range(len(sizes)) if c < sizes[g][1]]
    half = len(inter) // 2
    tw.cons(inter[:half])
    tw.compare("first half of the constraints")
    mask = [int(i % 11 != 3) for i in range(len(inter) - half)]
    tw.cons(inter[half:], mask=mask)
    tw.cons([r for r, keep in zip(inter[half:], mask) if not keep])  # the rows masked out, after all
    tw.compare("constraints")
    assert [tw.sd.counts(g) for g in range(len(sizes))] == sizes
    # graph 6: ids different from indices, a duplicated id (the last wins), an unknown id, two ids of one node,
    # id0 == id1, three constraints on one unordered pair in both directions
    g = len(sizes)
    tw.nodes([(g, 50, [0, 0, 0]), (g, 40, [1, 0, 0]), (g, 50, [2, 0, 0.1]), (g, 30, [3, 0, 0]), (g, 40, [4, 0.2, 0])])
    m3, k9 = np.array([1.0, 0.0, 0.0]), PREC
    add, st = tw.cons([(g, 50, 40, m3, k9), (g, 40, 50, -m3, k9), (g, 50, 999, m3, k9), (g, 40, 40, m3, k9), (g, 50, 40, m3, k9),
                       (g, 30, 50, m3, k9), (g, 30, 40, m3, k9)])
    assert add == [1, 1, 0, 0, 1, 1, 1] and st == [0, 0, 0, sp.SPA_EINVAL, 0, 0, 0]
    d = tw.sd.download_graph(g)
    assert d["ends"].tolist() == [[2, 4], [4, 2], [2, 4], [3, 2], [3, 4]]  # the LAST node with id 50 / 40
    assert d["pair_off"].tolist() == [0, 1, 4, 5] and d["pair_con"].tolist() == [3, 0, 1, 2, 4]
    tw.compare("ids")
    # capacity: graph 5 is full of nodes and of constraints
    assert tw.nodes([(5, 1, [0, 0, 0]), (0, 2000, [1, 1, 0])]) == [sp.SPA_ERANGE, 0]
    add, st = tw.cons([(5, 1000, 997, m3, k9), (0, 1000, 2000, m3, k9)])
    assert add == [0, 1] and st == [sp.SPA_ERANGE, 0]
    tw.compare("capacity")
    assert tw.sd.edit_info() == (3, sp.SPA_EINVAL)
    for solver in ("pcg", "cholesky"):
        tw.compare_compute(solver, "directed")
    tw.close()


def test_spa_contexts_beyond_the_limit_are_refused(gpu):
    f = sp.SpaFleet(1, sp.SPA_EDIT_MAX_NODES + 1, 8)
    with pytest.raises(sp.Slam2dError, match="-5"):
        f.edit_nodes_device(0, 0)
    with pytest.raises(sp.Slam2dError, match="-5"):
        f.edit_constraints_device(1, dev(np.zeros(1, sp.CON_ROW_DTYPE)).data_ptr())
    f.close()


# ------------------------------------------------------------------------------------ 3. random twin
def test_random_twin(gpu):
    rng = np.random.default_rng(11)
    G, N, M = 6, 48, 80
    tw = Twin(G, N, M, factor=N * (N + 1) // 2)
    poses = rng.uniform(-3, 3, (G, N, 3))
    for f in (tw.fd, tw.fh):
        for g in range(G):
            f.set_scans(g, 0, np.full((N, 8), 2.0), poses[g])

    def edge_rows():
        rows = []
        for g in range(G):
            n = tw.fh.counts(g)[0]
            for _ in range(int(rng.integers(0, 5))):
                kind = rng.integers(0, 10)
                if n < 2 or kind == 0:
                    rows.append((g, int(rng.integers(0, n + 2)), int(rng.integers(0, n + 2))))  # often refused
                elif kind < 4 and n >= 2:
                    rows.append((g, n - 1, n - 2))  # the link to the previous scan, repeated over the rounds
                else:
                    a = int(rng.integers(0, n))
                    rows.append((g, a, int((a + 1 + rng.integers(0, n - 1)) % n)))
        rng.shuffle(rows)
        return [tuple(int(v) for v in r) for r in rows] or [(-1, 0, 0)]

    def searches():
        q = [(g, max(tw.fh.counts(g)[0] - 1, 0), 0, -1, -1) for g in range(G)]
        return q, dev(kl.queries(q))

    for rnd in range(25):
        vrows = [(g, tw.fh.counts(g)[0] if rng.integers(0, 8) else 1 + tw.fh.counts(g)[0]) for g in range(G) if rng.integers(0, 4)]
        vrows = vrows or [(-1, -1)]
        # ---- enqueue: vertices, edges, search, edges, search -- no call that waits in between
        check_v = tw.vertices(vrows, enqueue_only=True)
        rows1 = edge_rows()
        new1, d_new1, check_e1 = tw.edges(rows1, enqueue_only=True)
        q1, d_q1 = searches()
        tw.fd.search_device(G, d_q1.data_ptr())
        rows2 = edge_rows()
        new2, d_new2, check_e2 = tw.edges(rows2, enqueue_only=True)
        q2, d_q2 = searches()
        tw.fd.search_device(G, d_q2.data_ptr())
        # ---- now read
        check_v(), check_e1(), check_e2()
        tw.fh.search(q2)
        for slot in range(G):
            same(tw.fd.get(slot), tw.fh.get(slot), f"round {rnd} search slot {slot}")
        # ---- the optimiser's side: a node per vertex the twin has more of, a constraint per new edge
        nrows = []
        for g in range(G):
            for k in range(tw.sh.counts(g)[0], tw.fh.counts(g)[0]):
                nrows.append((g, k, poses[g, k]))
        if nrows:
            tw.nodes(nrows)
        for rows, new, d_new in ((rows1, new1, d_new1), (rows2, new2, d_new2)):
            crow = [(g, s, t, rng.normal(size=3) * 0.2, PREC) for g, s, t in rows]
            tw.cons(crow, mask=new, d_mask=d_new)  # the is_new array itself is the mask
        tw.compare(f"round {rnd}")
    assert tw.seen["old"] >= 10 and tw.seen["new"] >= 10 and tw.seen["refused"] >= 3, tw.seen
    tw.compare_compute("pcg", "random twin")
    tw.close()


# ------------------------------------------------------------------------------------ 4. mixed host / device
def test_mixed_host_and_device_edits(gpu):
    tw = Twin(2, 8, 16)
    tw.vertices([(0, -1), (1, -1), (0, -1), (0, -1), (1, -1)])
    tw.nodes([(0, 0, [0, 0, 0]), (1, 0, [0, 0, 0]), (0, 1, [1, 0, 0]), (0, 2, [2, 0, 0]), (1, 1, [1, 1, 0])])
    tw.edges([(0, 1, 0), (1, 1, 0)])
    tw.cons([(0, 1, 0, [-1.0, 0, 0], PREC), (1, 1, 0, [-1.0, -1.0, 0], PREC)])
    # the host's copies follow the device
    assert tw.fd.counts(0) == (3, 1) == tw.fh.counts(0) and tw.sd.counts(1) == (2, 1)
    ids, poses = tw.sd.get_nodes(0)
    assert ids.tolist() == [0, 1, 2] and poses.tolist() == [[0, 0, 0], [1, 0, 0], [2, 0, 0]]
    assert tw.sd.device_poses(0)[1] == 3 and tw.sd.envelope_blocks(0, 1) == tw.sh.envelope_blocks(0, 1)
    # host edits on top (pull-back), on both fleets alike
    for f, s in ((tw.fd, tw.sd), (tw.fh, tw.sh)):
        assert f.add_edge(0, 2, 1) and not f.add_edge(0, 1, 0)
        assert s.add_constraint(0, 2, 1, [-1.0, 0, 0], PREC)
        assert f.add_vertex(1) == 2
        s.add_node(1, 2, [2.0, 1.0, 0.0])
    # and device edits again: the pending host edits are uploaded first
    tw.vertices([(0, 3), (1, 3)])
    tw.nodes([(0, 3, [3, 0, 0]), (1, 3, [3, 1, 0])])
    new, d_new, _ = tw.edges([(0, 2, 1), (0, 3, 2), (1, 3, 2), (1, 2, 1)])
    assert new == [0, 1, 1, 1]
    tw.cons([(0, 2, 1, [9, 9, 9], PREC), (0, 3, 2, [-1.0, 0, 0], PREC), (1, 3, 2, [-1.0, 0, 0], PREC), (1, 2, 1, [-1.0, 0, 0], PREC)],
            mask=new, d_mask=d_new)
    tw.compare("mixed")
    tw.compare_compute("pcg", "mixed")
    # set_graph and clear_graph overwrite a graph the device edited
    for f in (tw.fd, tw.fh):
        f.set_graph(0, 3, [(0, 2)])
        f.clear_graph(1)
    tw.edges([(0, 0, 2), (0, 2, 0)])
    tw.compare("overwritten")
    tw.close()


# ------------------------------------------------------------------------------------ 5. fleet replay
def test_fleet_replay_with_device_commits(gpu, monkeypatch):
    """test_karto_process_gpu.py::test_fleet_replay, its world and every assertion, with kp_commit_vertices and ke_commit
    replaced by kd_commit_vertices_device and kd_commit_edges_device."""
    import test_karto_process_gpu as T

    monkeypatch.setenv("SLAM2D_POISON", "1")
    edits = kd.GraphEdits(2 * 8)
    used = dict(vertices=0, edges=0)

    def commit_vertices(self, loop_fleet, spa_fleet):
        T.sync()  # the stages run on their own streams here
        edits.commit_vertices_device(self.result_device()["intake"], 0, 2, loop_fleet, spa_fleet)
        n_vertices, _, refused = edits.info()
        assert refused == 0
        used["vertices"] += n_vertices
        return n_vertices

    def commit(self, loop_fleet, spa_fleet, first_job, count):
        T.sync()
        r = self.result_device()
        edits.commit_edges_device(r["jobs_out"], r["links"], r["max_links"], first_job, count, loop_fleet, spa_fleet)
        _, n_new, refused = edits.info()
        assert refused == 0
        used["edges"] += n_new
        return n_new

    monkeypatch.setattr(kp.ProcessStage, "commit_vertices", commit_vertices)
    monkeypatch.setattr(ke.LinkStage, "commit", commit)
    T.test_fleet_replay(True)
    assert used["vertices"] >= 16 and used["edges"] >= 14, used
    edits.close()


# ------------------------------------------------------------------------------------ 6. one large graph
def test_one_large_graph_in_chunks(gpu):
    n = 4096
    tw = Twin(1, n, n + n // 16 + 8)
    rng = np.random.default_rng(3)
    pose = lambda k: [np.cos(2 * np.pi * k / n) * 50, np.sin(2 * np.pi * k / n) * 50, 2 * np.pi * k / n]  # noqa: E731
    for c in range(0, n, 512):
        tw.vertices([(0, k) for k in range(c, c + 512)])
        tw.nodes([(0, k, pose(k)) for k in range(c, c + 512)])
    edges = []
    for k in range(1, n):
        edges.append((0, k, k - 1))
        if k % 16 == 0:
            edges.append((0, k, (k + n // 2) % n))  # a closure edge every 16 scans
    edges.append((0, 0, n - 1))
    edges.append((0, 1, 0))  # old
    for c in range(0, len(edges), 512):
        part = edges[c:c + 512]
        new, d_new, _ = tw.edges(part)
        tw.cons([(0, s, t, rng.normal(size=3), PREC) for _, s, t in part], mask=new, d_mask=d_new)
    tw.compare("large")
    assert tw.fd.counts(0) == (n, len(edges) - 1) and tw.sd.counts(0) == (n, len(edges) - 1)
    tw.close()


# ------------------------------------------------------------------------------------ 7. the stage's own rules
def test_kd_rules_counts_and_timing(gpu):
    """kp_plan_vertices' and ke_plan_commit's rules on hand-made records: which records become rows, first_job, the
    link cap, the totals of kd_get_info and the stage's launch counts."""
    tw = Twin(4, 6, 8)
    edits = kd.GraphEdits(12)
    edits.set_timing(True)

    def intake(rows):
        rec = np.zeros(4, kp.INTAKE_DTYPE)
        for i, (accepted, status, scan) in enumerate(rows):
            rec[i]["accepted"], rec[i]["status"], rec[i]["scan"] = accepted, status, scan
            rec[i]["corrected"] = [0.5 * scan, 0.1 * i, 0.01 * scan]
        d = dev(rec)
        edits.commit_vertices_device(d.data_ptr(), 0, 4, tw.fd, tw.sd)
        return rec, edits.info()

    # accepted; not accepted; accepted but refused by the intake; accepted with a scan index the graph does not have
    rec, info = intake([(1, 0, 0), (0, 0, 0), (1, kp.KP_ERANGE, 0), (1, 0, 5)])
    assert info == (1, 0, 1)
    assert tw.fh.add_vertex(0) == 0
    tw.sh.add_node(0, 0, rec[0]["corrected"])
    tw.compare("first intake")
    for scan0, scan3 in ((1, 0), (2, 1)):
        rec, info = intake([(1, 0, scan0), (0, 0, 0), (0, 0, 0), (1, 0, scan3)])
        assert info == (2, 0, 0)
        for g, s in ((0, scan0), (3, scan3)):
            assert tw.fh.add_vertex(g) == s
            tw.sh.add_node(g, s, rec[0 if g == 0 else 3]["corrected"])
    tw.compare("intakes")
    # job 0 lies before first_job; job 1: a new edge, a singular record, the same edge again (old); job 2 has a status
    # that commits nothing; job 3 (KE_SINGULAR, n_links beyond max_links): two new edges and an end that is no vertex
    K = 3
    jobs, links = np.zeros(4, ke.JOB_OUT_DTYPE), np.zeros((4, K), ke.LINK_DTYPE)
    plan = [(ke.KE_OK, 1, 1, [(0, 1, 0)]),
            (ke.KE_OK, 3, 0, [(2, 1, 0), (2, 0, ke.KE_SINGULAR), (2, 1, 0)]),
            (ke.KE_ERANGE, 2, 0, [(1, 0, 0), (2, 0, 0)]),
            (ke.KE_SINGULAR, 5, 0, [(1, 0, 0), (0, 1, 0), (1, 5, 0)])]
    rng = np.random.default_rng(5)
    for j, (status, n_links, graph, recs) in enumerate(plan):
        jobs[j]["status"], jobs[j]["n_links"], jobs[j]["graph"] = status, n_links, graph
        for r, (a, b, st) in enumerate(recs):
            links[j, r]["from"], links[j, r]["to"], links[j, r]["status"] = a, b, st
            links[j, r]["diff"], links[j, r]["precision"] = rng.normal(size=3), (PREC + r * np.eye(3)).reshape(9)
    d_jobs, d_links = dev(jobs), dev(links)
    edits.commit_edges_device(d_jobs.data_ptr(), d_links.data_ptr(), K, 1, 3, tw.fd, tw.sd)
    assert edits.info() == (0, 3, 1)
    for j, r in ((1, 0), (3, 0), (3, 1)):
        l_ = links[j, r]
        assert tw.fh.add_edge(0, int(l_["from"]), int(l_["to"]))
        assert tw.sh.add_constraint(0, int(l_["from"]), int(l_["to"]), l_["diff"], l_["precision"])
    tw.compare("edges")
    assert tw.fd.edit_info() == (2, kl.KL_EINVAL) and tw.sd.edit_info() == (0, 0)
    t = edits.kernel_times()
    assert [t[k][1] for k in ("kd_flatten_vertices_kernel", "kd_flatten_edges_kernel", "kd_tally_kernel")] == [3, 1, 8]
    assert all(v[0] > 0.0 for v in t.values())
    with pytest.raises(kd.Slam2dError) as e:
        edits.commit_edges_device(d_jobs.data_ptr(), d_links.data_ptr(), K, 0, 5, tw.fd, tw.sd)
    assert e.value.code == kd.KD_ERANGE
    edits.close()
    tw.close()
