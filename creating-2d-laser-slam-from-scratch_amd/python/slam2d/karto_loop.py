"""Karto's loop-closure and near-chain candidate search over the MI355X C-ABI (include/slam2d/karto_loop.h).

Reference: MapperGraph::FindNearLinkedScans, FindPossibleLoopClosure, FindNearChains, GetClosestScanToPose /
LinkChainToScan (lesson6/lib/open_karto/src/Mapper.cpp:1054-1073, :1152-1286, :1333-1394) on the reference poses of
LocalizedRangeScan::Update (Karto.h:5362-5416), for a fleet of device-resident graphs: `LoopSearchFleet` mirrors the
kl_* entry points one to one.  Results are checked against tests/ref/karto_loop_ref.c (parity unpinned against the
compiled library: open_karto needs boost).  One sensor only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib  # noqa: F401  (callers reach the library through the module)
from ._lib import Slam2dError  # noqa: F401
from ._stage import TimedStage, dp as _dp, hp as _hp, library, params_from
from .karto import KtLaser

KL_OK, KL_EINVAL, KL_EHIP, KL_ENOMEM, KL_ENODEV, KL_ERANGE = 0, -1, -2, -3, -4, -5
KL_MAX_SCANS = 4096
KL_LOOP_CHAINS, KL_NEAR_CHAINS = 0, 1
KL_CHAIN_LONG, KL_CHAIN_LINKED = 1, 2
KL_EMIT_OVERFLOW = 1


class KlParams(C.Structure):
    _fields_ = [("link_scan_maximum_distance", C.c_double), ("loop_search_maximum_distance", C.c_double),
                ("loop_match_minimum_chain_size", C.c_int), ("use_scan_barycenter", C.c_int)]


class KlResult(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("status", "n_scans", "n_near_link", "n_near_loop", "n_loop_chains",
                                       "n_near_chains", "loop_index_total", "n_near_long", "near_index_total", "pad_")]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


QUERY_DTYPE = np.dtype([(k, np.int32) for k in ("graph", "scan", "start_num", "n_scans", "n_edges")])
RESULT_DTYPE = np.dtype([(k, np.int32) for k, _ in KlResult._fields_])
LOOP_CHAIN_DTYPE = np.dtype([(k, np.int32) for k in ("begin", "length", "resume", "pad_")])
NEAR_CHAIN_DTYPE = np.dtype([(k, np.int32) for k in ("begin", "length", "closest", "flags")])
CLOSEST_ITEM_DTYPE = np.dtype([(k, np.int32) for k in ("graph", "scan", "begin", "length")])
CLOSEST_DTYPE = np.dtype([(k, np.int32) for k in ("closest", "linked")])
SOURCE_DTYPE = np.dtype([(k, np.int32) for k in ("slot", "chain")])
EDGE_ROW_DTYPE = np.dtype([(k, np.int32) for k in ("graph", "source", "target", "pad_")])
REFRESH_ROW_DTYPE = np.dtype([(k, np.int32) for k in ("graph", "first", "count", "pool_first")])
REFRESH_SPAN_DTYPE = np.dtype([(k, np.int32) for k in ("pool_first", "count")])
KL_REFRESH_MAX_ROWS = 4096


class KlEdgeRow(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("graph", "source", "target", "pad_")]


def _declare(L):
    if getattr(L, "_kl_declared", False):
        return
    vp, i, P = C.c_void_p, C.c_int, C.POINTER
    L.kl_last_error.restype = C.c_char_p
    L.kl_version.restype = C.c_char_p
    L.kl_default_params.restype = None
    L.kl_default_params.argtypes = [P(KlParams)]
    L.kl_node_params.restype = None
    L.kl_node_params.argtypes = [P(KlParams)]
    L.kl_create.argtypes = [P(vp), P(KtLaser), P(KlParams), i, i, i, i]
    L.kl_destroy.argtypes = [vp]
    L.kl_add_vertex.argtypes = [vp, i, P(i)]
    L.kl_add_edge.argtypes = [vp, i, i, i, P(i)]
    L.kl_set_graph.argtypes = [vp, i, i, i, vp]
    L.kl_clear_graph.argtypes = [vp, i]
    L.kl_get_counts.argtypes = [vp, i, P(i), P(i)]
    L.kl_set_pool_offset.argtypes = [vp, i, i]
    L.kl_set_scans.argtypes = [vp, i, i, i, vp, vp]
    L.kl_set_scans_device.argtypes = [vp, i, i, i, vp, vp, vp]
    L.kl_get_reference.argtypes = [vp, i, i, i, vp]
    L.kl_refresh_device.argtypes = [vp, i, vp, vp, vp, i, vp, vp]
    L.kl_get_refresh_info.argtypes = [vp, P(i), P(i)]
    L.kl_search.argtypes = [vp, i, vp]
    L.kl_search_device.argtypes = [vp, i, vp, vp]
    L.kl_get_result.argtypes = [vp, i, P(KlResult)]
    L.kl_get_d2.argtypes = [vp, i, vp]
    L.kl_get_near.argtypes = [vp, i, vp, vp]
    L.kl_get_chains.argtypes = [vp, i, vp, vp]
    L.kl_result_device.argtypes = [vp, P(vp), P(vp), P(vp), P(vp), P(vp), P(vp), P(i)]
    L.kl_closest_device.argtypes = [vp, i, vp, vp, vp]
    L.kl_emit_batch_device.argtypes = [vp, i, i, i, vp, vp, vp, vp, vp, vp]
    L.kl_get_emit_info.argtypes = [vp, P(i), P(i)]
    L.kl_edit_vertices_device.argtypes = [vp, i, vp, vp, vp, vp, vp]
    L.kl_edit_edges_device.argtypes = [vp, i, vp, vp, vp, vp]
    L.kl_get_edit_info.argtypes = [vp, P(i), P(i)]
    L.kl_download_graph.argtypes = [vp, i, P(i), P(i), vp, vp, vp]
    L.kl_set_timing.argtypes = [vp, i]
    L.kl_num_kernels.restype = i
    L.kl_kernel_name.restype = C.c_char_p
    L.kl_kernel_name.argtypes = [i]
    L.kl_get_kernel_times.argtypes = [vp, vp, vp, i]
    L._kl_declared = True


def default_params(**kw) -> KlParams:
    """kl_default_params: the Mapper defaults (link 10.0, loop 4.0, chain size 10, barycentre on); keywords override."""
    return params_from(library(_declare), KlParams, "kl_default_params", **kw)


def node_params(**kw) -> KlParams:
    """kl_node_params: mapper_params.yaml (link 1.5, loop 10.0, chain size 5, barycentre on); keywords override."""
    return params_from(library(_declare), KlParams, "kl_node_params", **kw)


def queries(rows) -> np.ndarray:
    """rows of (graph, scan, start_num, n_scans, n_edges) -> a kl_query array."""
    a = np.ascontiguousarray(rows, np.int32).reshape(-1, 5)
    return np.ascontiguousarray(a).view(QUERY_DTYPE).reshape(-1)


class LoopSearchFleet(TimedStage):
    """`max_graphs` graphs of up to `max_scans` (<= KL_MAX_SCANS) scans and `max_edges` edges, device resident, and
    result slots for `max_queries` queries per search; one workgroup answers each query."""

    _PREFIX = "kl"

    def __init__(self, laser: KtLaser, params: KlParams | None, max_graphs: int, max_scans: int, max_edges: int,
                 max_queries: int):
        self.L = library(_declare)
        self.laser = laser
        self.params = params if params is not None else default_params()
        self.max_graphs, self.max_scans = int(max_graphs), int(max_scans)
        self.max_edges, self.max_queries = int(max_edges), int(max_queries)
        self.h = C.c_void_p()
        self._check(self.L.kl_create(C.byref(self.h), C.byref(laser), C.byref(self.params), self.max_graphs,
                                     self.max_scans, self.max_edges, self.max_queries), "kl_create")

    # ------------------------------------------------------------------------------------------------ the graph
    def add_vertex(self, g: int) -> int:
        sid = C.c_int(-1)
        self._check(self.L.kl_add_vertex(self.h, g, C.byref(sid)), "kl_add_vertex")
        return sid.value

    def add_edge(self, g: int, source: int, target: int) -> bool:
        """AddEdge's rIsNewEdge."""
        new = C.c_int(0)
        self._check(self.L.kl_add_edge(self.h, g, int(source), int(target), C.byref(new)), "kl_add_edge")
        return bool(new.value)

    def set_graph(self, g: int, n_scans: int, ends):
        e = np.ascontiguousarray(ends, np.int32).reshape(-1, 2)
        self._check(self.L.kl_set_graph(self.h, g, int(n_scans), len(e), _hp(e)), "kl_set_graph")

    def clear_graph(self, g: int):
        self._check(self.L.kl_clear_graph(self.h, g), "kl_clear_graph")

    def counts(self, g: int):
        n, m = C.c_int(0), C.c_int(0)
        self._check(self.L.kl_get_counts(self.h, g, C.byref(n), C.byref(m)), "kl_get_counts")
        return n.value, m.value

    def set_pool_offset(self, g: int, offset: int):
        self._check(self.L.kl_set_pool_offset(self.h, g, int(offset)), "kl_set_pool_offset")

    # ------------------------------------------------------------------------------------------------ reference poses
    def set_scans(self, g: int, first: int, ranges, poses):
        po = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        r = np.ascontiguousarray(ranges, np.float64).reshape(len(po), self.laser.n_readings)
        self._check(self.L.kl_set_scans(self.h, g, int(first), len(po), _hp(r), _hp(po)), "kl_set_scans")

    def set_scans_device(self, g: int, first: int, count: int, d_ranges: int, d_poses: int, hip_stream: int = 0):
        self._check(self.L.kl_set_scans_device(self.h, g, int(first), int(count), _dp(d_ranges), _dp(d_poses),
                                               _dp(hip_stream)), "kl_set_scans_device")

    def get_reference(self, g: int, first: int = 0, count: int | None = None) -> np.ndarray:
        count = self.counts(g)[0] - first if count is None else count
        out = np.zeros((count, 2), np.float64)
        self._check(self.L.kl_get_reference(self.h, g, int(first), int(count), _hp(out)), "kl_get_reference")
        return out

    def refresh_device(self, n_rows: int, d_rows: int, d_pool_ranges: int, d_pool_poses: int, pool_scans: int,
                       d_resolved: int = 0, hip_stream: int = 0):
        """kl_refresh_device: `n_rows` kl_refresh_row rows (REFRESH_ROW_DTYPE) at device address d_rows; d_resolved
        gets REFRESH_SPAN_DTYPE rows."""
        self._check(self.L.kl_refresh_device(self.h, int(n_rows), _dp(d_rows), _dp(d_pool_ranges), _dp(d_pool_poses),
                                             int(pool_scans), _dp(d_resolved), _dp(hip_stream)), "kl_refresh_device")

    def refresh_info(self):
        """(rows kl_refresh_device refused since the last call, status of the first); waits."""
        n, st = C.c_int(0), C.c_int(0)
        self._check(self.L.kl_get_refresh_info(self.h, C.byref(n), C.byref(st)), "kl_get_refresh_info")
        return n.value, st.value

    # ------------------------------------------------------------------------------------------------ the search
    def search(self, rows):
        """rows of (graph, scan, start_num, n_scans, n_edges); waits for the results."""
        q = queries(rows)
        self._check(self.L.kl_search(self.h, len(q), _hp(q)), "kl_search")
        return len(q)

    def search_device(self, count: int, d_queries: int, hip_stream: int = 0):
        self._check(self.L.kl_search_device(self.h, int(count), _dp(d_queries), _dp(hip_stream)), "kl_search_device")

    def result(self, slot: int) -> dict:
        r = KlResult()
        self._check(self.L.kl_get_result(self.h, int(slot), C.byref(r)), "kl_get_result")
        return r.as_dict()

    def get(self, slot: int) -> dict:
        """Everything slot `slot` holds: the counts, d2, near_link, near_loop, loop_chains [k, 3] = begin, length,
        resume, near_chains [k, 4] = begin, length, closest, flags."""
        out = self.result(slot)
        d2 = np.zeros(max(out["n_scans"], 0), np.float64)
        nl, no = np.zeros(out["n_near_link"], np.int32), np.zeros(out["n_near_loop"], np.int32)
        lc, nc = np.zeros((out["n_loop_chains"], 4), np.int32), np.zeros((out["n_near_chains"], 4), np.int32)
        self._check(self.L.kl_get_d2(self.h, int(slot), _hp(d2)), "kl_get_d2")
        self._check(self.L.kl_get_near(self.h, int(slot), _hp(nl), _hp(no)), "kl_get_near")
        self._check(self.L.kl_get_chains(self.h, int(slot), _hp(lc), _hp(nc)), "kl_get_chains")
        out.update(d2=d2, near_link=nl, near_loop=no, loop_chains=lc[:, :3].copy(), near_chains=nc)
        return out

    def result_device(self) -> dict:
        """Device addresses of the result arrays and the chain arrays' stride."""
        ptrs = [C.c_void_p() for _ in range(6)]
        stride = C.c_int(0)
        self._check(self.L.kl_result_device(self.h, *[C.byref(p) for p in ptrs], C.byref(stride)), "kl_result_device")
        names = ("results", "d2", "near_link", "near_loop", "loop_chains", "near_chains")
        out = {k: int(p.value or 0) for k, p in zip(names, ptrs)}
        out["chain_stride"] = stride.value
        return out

    def closest_device(self, count: int, d_items: int, d_out: int, hip_stream: int = 0):
        self._check(self.L.kl_closest_device(self.h, int(count), _dp(d_items), _dp(d_out), _dp(hip_stream)),
                    "kl_closest_device")

    def emit_batch_device(self, count: int, which: int, capacity: int, d_query: int, d_base_begin: int,
                          d_base_index: int, d_source: int, d_n_matches: int, hip_stream: int = 0):
        self._check(self.L.kl_emit_batch_device(self.h, int(count), int(which), int(capacity), _dp(d_query),
                                                _dp(d_base_begin), _dp(d_base_index), _dp(d_source), _dp(d_n_matches),
                                                _dp(hip_stream)), "kl_emit_batch_device")

    def emit_info(self):
        """(matches before the capacity cut, status) of the last emit."""
        total, status = C.c_int(0), C.c_int(0)
        self._check(self.L.kl_get_emit_info(self.h, C.byref(total), C.byref(status)), "kl_get_emit_info")
        return total.value, status.value

    # ------------------------------------------------------------------------------------------------ device edits
    def edit_vertices_device(self, count: int, d_graph: int, d_expect_id: int = 0, d_id: int = 0, d_status: int = 0,
                             hip_stream: int = 0):
        """kl_edit_vertices_device: row i adds a vertex to graph d_graph[i] (device int array)."""
        self._check(self.L.kl_edit_vertices_device(self.h, int(count), _dp(d_graph), _dp(d_expect_id), _dp(d_id),
                                                   _dp(d_status), _dp(hip_stream)), "kl_edit_vertices_device")

    def edit_edges_device(self, count: int, d_rows: int, d_is_new: int = 0, d_status: int = 0, hip_stream: int = 0):
        """kl_edit_edges_device: `count` kl_edge_row rows (EDGE_ROW_DTYPE) at device address d_rows."""
        self._check(self.L.kl_edit_edges_device(self.h, int(count), _dp(d_rows), _dp(d_is_new), _dp(d_status),
                                                _dp(hip_stream)), "kl_edit_edges_device")

    def edit_info(self):
        """(rows refused since the last call, status of the first); waits."""
        n, st = C.c_int(0), C.c_int(0)
        self._check(self.L.kl_get_edit_info(self.h, C.byref(n), C.byref(st)), "kl_get_edit_info")
        return n.value, st.value

    def download_graph(self, g: int) -> dict:
        """Graph g's DEVICE arrays (pending host edits are uploaded first): n_scans, n_edges, ends [m, 2], adj_off
        [n + 1], adj [2m, 2] = other end, edge index."""
        n, m = C.c_int(0), C.c_int(0)
        self._check(self.L.kl_download_graph(self.h, g, C.byref(n), C.byref(m), None, None, None), "kl_download_graph")
        n, m = n.value, m.value
        ends, off, adj = np.zeros((m, 2), np.int32), np.zeros(n + 1, np.int32), np.zeros((2 * m, 2), np.int32)
        self._check(self.L.kl_download_graph(self.h, g, None, None, _hp(ends), _hp(off), _hp(adj)), "kl_download_graph")
        return {"n_scans": n, "n_edges": m, "ends": ends, "adj_off": off, "adj": adj}
