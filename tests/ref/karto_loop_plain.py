"""A literal Python transcription of open_karto's loop-closure and near-chain candidate search, member by member, for
the tests: none of the run or batch reformulations of include/slam2d/karto_loop.h appears here.

  Vertex, Edge, Graph.AddEdge         Mapper.h:251-272, :304-309; Mapper.cpp:1075-1101
  traverse                            BreadthFirstTraversal::Traverse, Mapper.h:568-612 (queue and seen set)
  NearScanVisitor                     Mapper.h:619-643
  find_near_linked_scans              Mapper.cpp:1278-1286
  find_possible_loop_closure          Mapper.cpp:1333-1394 (the rStartNum loop), driven by loop_chains' while
                                      (!chain.empty()) loop, the caller's at Mapper.cpp:984-1048 with no closure accepted
  find_near_chains                    Mapper.cpp:1170-1275 (the processed vector and the two for loops)
  get_closest_scan_to_pose, link_test Mapper.cpp:1054-1073, :1152-1167
  barycenter                          LocalizedRangeScan::Update, Karto.h:5362-5416: the point readings come from the C
                                      restatement (detmath's sin / cos), the sum is Python's, one point at a time
Test infrastructure: nothing here is imported by the package.
"""
from __future__ import annotations

from collections import deque

import karto_loop_ref as R

KT_TOLERANCE = 1e-06
DBL_MAX = 1.7976931348623157e308


def square(v):
    return v * v


def squared_distance(a, b):
    """Vector2::SquaredDistance (Karto.h:1011-1032): (*this - rOther).SquaredLength()."""
    dx, dy = a[0] - b[0], a[1] - b[1]
    return square(dx) + square(dy)


class Vertex:
    def __init__(self, obj):
        self.obj = obj  # the scan's state id
        self.edges = []

    def adjacent(self):
        out = []
        for e in self.edges:
            if e.source is not self:
                out.append(e.source)
            if e.target is not self:
                out.append(e.target)
        return out


class Edge:
    def __init__(self, source, target):
        self.source, self.target = source, target
        source.edges.append(self)
        target.edges.append(self)


class Graph:
    """One sensor's MapperGraph over scans with reference positions `ref`."""

    def __init__(self):
        self.vertices = []
        self.edges = []

    def add_vertex(self):
        self.vertices.append(Vertex(len(self.vertices)))
        return len(self.vertices) - 1

    def add_edge(self, source: int, target: int):
        """AddEdge: (edge, is_new)."""
        v1, v2 = self.vertices[source], self.vertices[target]
        for e in v1.edges:
            if e.target is v2:
                return e, False
        e = Edge(v1, v2)
        self.edges.append(e)
        return e, True

    def append_edge(self, source: int, target: int):
        """new Edge(v1, v2) without AddEdge's lookup (kl_set_graph's bulk form)."""
        self.edges.append(Edge(self.vertices[source], self.vertices[target]))


def graph_of(n_scans: int, ends) -> Graph:
    g = Graph()
    for _ in range(n_scans):
        g.add_vertex()
    for s, t in ends:
        g.append_edge(int(s), int(t))
    return g


def barycenter(laser: dict, use_barycenter: int, ranges, pose):
    """GetReferencePose(useBarycenter)'s position after Update()."""
    if not use_barycenter:
        return (float(pose[0]), float(pose[1]))
    px, py, ok = R.points(laser, ranges, pose)
    sx, sy, cnt = 0.0, 0.0, 0
    for i in range(len(px)):
        if not ok[i]:
            continue
        sx += float(px[i])
        sy += float(py[i])
        cnt += 1
    n_points = float(cnt)
    if n_points != 0.0:
        return (sx / n_points, sy / n_points)
    return (float(pose[0]), float(pose[1]))


def traverse(start: Vertex, visit):
    to_visit = deque([start])
    seen = {start}
    valid = []
    while True:
        nxt = to_visit.popleft()
        if visit(nxt):
            valid.append(nxt)
            for adj in nxt.adjacent():
                if adj not in seen:
                    to_visit.append(adj)
                    seen.add(adj)
        if not to_visit:
            break
    return [v.obj for v in valid]


def find_near_linked_scans(g: Graph, ref, scan: int, max_distance: float):
    max_d2 = square(max_distance)
    center = ref[scan]

    def visit(v):
        return squared_distance(ref[v.obj], center) <= max_d2 - KT_TOLERANCE

    return traverse(g.vertices[scan], visit)


def find_possible_loop_closure(g: Graph, ref, scan: int, start_num: int, loop: float, min_chain: int):
    """(chain, rStartNum after the call)."""
    chain = []
    pose = ref[scan]
    near_linked = find_near_linked_scans(g, ref, scan, loop)
    n_scans = len(g.vertices)
    while start_num < n_scans:
        cand = start_num
        d2 = squared_distance(ref[cand], pose)
        if d2 < square(loop) + KT_TOLERANCE:
            if cand in near_linked:
                chain = []
            else:
                chain.append(cand)
        else:
            if len(chain) >= min_chain:
                return chain, start_num
            chain = []
        start_num += 1
    return chain, start_num


def loop_chains(g: Graph, ref, scan: int, start_num: int, loop: float, min_chain: int):
    """TryCloseLoop's loop with every candidate rejected: [(begin, length, resume), ...]."""
    out = []
    chain, start_num = find_possible_loop_closure(g, ref, scan, start_num, loop, min_chain)
    while chain:
        assert chain == list(range(chain[0], chain[0] + len(chain)))
        out.append((chain[0], len(chain), start_num))
        chain, start_num = find_possible_loop_closure(g, ref, scan, start_num, loop, min_chain)
    return out


def get_closest_scan_to_pose(ref, scans, pose):
    closest, best = None, DBL_MAX
    for s in scans:
        d2 = squared_distance(pose, ref[s])
        if d2 < best:
            best = d2
            closest = s
    return closest


def link_test(ref, chain, scan: int, link: float):
    """LinkChainToScan up to its LinkScans call: (closest, linked)."""
    pose = ref[scan]
    closest = get_closest_scan_to_pose(ref, chain, pose)
    if closest is None:
        return -1, 0
    return closest, int(squared_distance(pose, ref[closest]) < square(link) + KT_TOLERANCE)


def find_near_chains(g: Graph, ref, scan: int, link: float):
    near_chains = []
    scan_pose = ref[scan]
    processed = []
    near_linked = find_near_linked_scans(g, ref, scan, link)
    for near in near_linked:
        if near == scan:
            continue
        if near in processed:
            continue
        processed.append(near)
        is_valid = True
        chain = deque()
        cand = near - 1
        while cand >= 0:
            if cand == scan:
                is_valid = False
            if squared_distance(scan_pose, ref[cand]) < square(link) + KT_TOLERANCE:
                chain.appendleft(cand)
                processed.append(cand)
            else:
                break
            cand -= 1
        chain.append(near)
        end = len(g.vertices)
        cand = near + 1
        while cand < end:
            if cand == scan:
                is_valid = False
            if squared_distance(scan_pose, ref[cand]) < square(link) + KT_TOLERANCE:
                chain.append(cand)
                processed.append(cand)
            else:
                break
            cand += 1
        if is_valid:
            near_chains.append(list(chain))
    return near_chains


def search(n_total: int, ends, ref, scan: int, start_num: int, link: float, loop: float, min_chain: int,
           n_scans: int = -1, n_edges: int = -1) -> dict:
    """What one kl_query produces, by the reference's members on the visible prefix of the graph."""
    n = n_total if n_scans < 0 else n_scans
    ends = [(int(s), int(t)) for s, t in ends]
    ne = len(ends) if n_edges < 0 else n_edges
    g = graph_of(n, [(s, t) for s, t in ends[:ne] if s < n and t < n])
    ref = [(float(x), float(y)) for x, y in ref][:n]
    out = {"d2": [squared_distance(ref[i], ref[scan]) for i in range(n)],
           "near_link": find_near_linked_scans(g, ref, scan, link),
           "near_loop": find_near_linked_scans(g, ref, scan, loop),
           "loop_chains": loop_chains(g, ref, scan, start_num, loop, min_chain), "near_chains": []}
    for chain in find_near_chains(g, ref, scan, link):
        assert chain == list(range(chain[0], chain[0] + len(chain)))
        closest, linked = link_test(ref, chain, scan, link)
        out["near_chains"].append((chain[0], len(chain), closest, (1 if len(chain) >= min_chain else 0) | 2 * linked))
    return out


def search_case(case: dict, query) -> dict:
    p = case["params"]
    ref = [barycenter(case["laser"], p["use_scan_barycenter"], r, po) for r, po in zip(case["ranges"], case["poses"])]
    scan, start, ns, ne = (int(v) for v in query)
    return search(len(case["poses"]), case["ends"], ref, scan, start, p["link_scan_maximum_distance"],
                  p["loop_search_maximum_distance"], p["loop_match_minimum_chain_size"], ns, ne)
