"""GPU parity of the record-indexed scan refresh and CorrectPoses (kl_refresh_device, kt_refresh_device,
spa_compute_rows_device, spa_export_poses_device and the kc_ stage that joins them) against the host-indexed entry
points of the same library in a TWIN context -- kl_set_scans_device, kt_set_scans_device, spa_compute, which the older
tests pin to the restatements -- and, for the reference positions, against tests/ref/karto_loop_ref.c directly.
Every comparison is by bytes; no tolerance appears anywhere."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "ref"))
import karto_loop_ref as LR  # noqa: E402
import spa2d_ref as SR  # noqa: E402

from slam2d import Slam2dError  # noqa: E402
from slam2d import karto as kt  # noqa: E402
from slam2d import karto_correct as kc  # noqa: E402
from slam2d import karto_edit as kd  # noqa: E402
from slam2d import karto_link as ke  # noqa: E402
from slam2d import karto_loop as kl  # noqa: E402
from slam2d import karto_process as kp  # noqa: E402
from slam2d import spa  # noqa: E402

pytestmark = pytest.mark.gpu

H2D, D2H = 1, 2
READINGS = [1, 63, 64, 65, 130]   # below, at and above one wave's 64 points; more than two passes
KNOB = [None, "1", "2"]           # SLAM2D_REFRESH_WG: the plan's grid, one workgroup, two


@functools.lru_cache(maxsize=None)
def _hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return h


def peek(ptr, dtype, shape):
    """Device memory at ptr as a host array (after a device synchronisation)."""
    import torch

    torch.cuda.synchronize()
    a = np.zeros(shape, dtype)
    if a.nbytes:
        assert _hip().hipMemcpy(a.ctypes.data_as(C.c_void_p), ptr, a.nbytes, D2H) == 0
    return a


def poke(ptr, a):
    import torch

    torch.cuda.synchronize()
    a = np.ascontiguousarray(a)
    assert _hip().hipMemcpy(ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, H2D) == 0


def dev(a):
    """The bytes of a host array on the device (spare bytes, so that an empty array still has an address)."""
    import torch

    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([b, np.zeros(16, np.uint8)])).cuda()


def host(t, dtype, n):
    return t.cpu().numpy()[:n * np.dtype(dtype).itemsize].copy().view(dtype)


def sync():
    import torch

    torch.cuda.synchronize()


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}\n{a}\n{b}"


@pytest.fixture
def knob(gpu, monkeypatch, request):
    """SLAM2D_REFRESH_WG before the contexts are created, and poisoned buffers, so that a scan no call ever set
    reads the same bytes in a context and in its twin."""
    monkeypatch.setenv("SLAM2D_POISON", "1")
    if request.param is None:
        monkeypatch.delenv("SLAM2D_REFRESH_WG", raising=False)
    else:
        monkeypatch.setenv("SLAM2D_REFRESH_WG", request.param)
    return request.param


def laser_dict(n):
    return dict(minimum_angle=-1.0, angular_resolution=2.1 / max(n, 2), minimum_range=0.1, range_threshold=4.0, n_readings=n)


def laser_of(n):
    d = laser_dict(n)
    return kt.laser(n, d["minimum_angle"], d["angular_resolution"], d["minimum_range"], d["range_threshold"])


def pool_of(n_slots, n, seed, dead=None):
    """Ranges with readings below the minimum, above the threshold, NaN and +-inf among them; slot `dead` has no valid
    reading at all.  Poses anywhere."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.2, 3.9, (n_slots, n))
    special = [0.05, 4.5, np.nan, np.inf, -np.inf, 0.1, 4.0]   # the last two are valid: InRange is inclusive
    for s in range(n_slots):
        for k, v in enumerate(special):
            i = (3 * s + 5 * k) % n
            if n > 1 or (s + k) % 3 == 0:
                r[s, i] = v
    if dead is not None:
        r[dead] = np.resize([np.nan, 4.5, 0.01, np.inf, -np.inf], n)
    p = np.stack([rng.uniform(-3, 3, n_slots), rng.uniform(-3, 3, n_slots), rng.uniform(-3.1, 3.1, n_slots)], axis=1)
    return np.ascontiguousarray(r), np.ascontiguousarray(p)


# ====================================================================================== 1. kl_refresh_device
KL_G, KL_N, KL_POOL = 3, 8, 16
KL_SCANS = (0, 1, 5)
KL_OFF = (0, 2, 4)     # graph g's scan i is pool slot KL_OFF[g] + i
# (graph, first, count, pool_first) and what the row resolves to, or the refusal's status
KL_ROWS = [
    ((1, 0, -1, 2), 1),                  # an open row over a whole graph
    ((0, 0, -1, 1), 0),                  # ... over an empty one
    ((2, 2, 2, 6), 2),                   # {g, 2, 2}
    ((-1, 0, 3, 0), None),               # skipped
    ((2, 0, 1, 4), 1),                   # a disjoint part of the same graph
    ((3, 0, 1, 0), kl.KL_EINVAL),        # graph >= max_graphs
    ((2, -1, 1, 0), kl.KL_EINVAL),       # first < 0
    ((2, 7, 2, 11), kl.KL_ERANGE),       # scans beyond max_scans
    ((2, 1, 1, 16), kl.KL_ERANGE),       # a pool slot >= pool_scans
    ((2, 3, -1, 7), 2),                  # open from scan 3: scans 3 and 4 (scan 3 again, from the same slot)
    ((2, 5, 3, 9), 3),                   # an explicit count is bounded by max_scans only: scans 5 .. 7
    ((1, 0, -1, 2), 1), ((2, 2, 2, 6), 2), ((2, 2, 3, 6), 3),   # named again: the same slots, the same values
    ((2, 8, 0, 0), 0), ((2, 0, 0, 16), 0),                       # nothing named: nothing to refuse
]
KL_UNNAMED = [(2, 1)]   # a scan of graph 2 no row names


def kl_fleet(n, bary):
    f = kl.LoopSearchFleet(laser_of(n), kl.default_params(use_scan_barycenter=bary), KL_G, KL_N, 4, 1)
    for g, cnt in enumerate(KL_SCANS):
        for _ in range(cnt):
            f.add_vertex(g)
    return f


@pytest.mark.parametrize("knob", KNOB, indirect=True)
@pytest.mark.parametrize("bary", [0, 1])
@pytest.mark.parametrize("n", READINGS)
def test_kl_refresh_equals_set_scans_and_the_restatement(knob, n, bary):
    assert sum(c for _, c in KL_ROWS if c and c > 0) == 15   # four waves per workgroup: the stride loop wraps
    ranges, poses0 = pool_of(KL_POOL, n, 100 + n, dead=7)
    _, poses1 = pool_of(KL_POOL, n, 200 + n)
    f, twin = kl_fleet(n, bary), kl_fleet(n, bary)
    for c in (f, twin):   # a first kl_set_scans of every scan, from the first poses
        for g in range(KL_G):
            if KL_SCANS[g]:
                c.set_scans(g, 0, ranges[KL_OFF[g]:KL_OFF[g] + KL_SCANS[g]], poses0[KL_OFF[g]:KL_OFF[g] + KL_SCANS[g]])
    before = [f.get_reference(g, 0, KL_N) for g in range(KL_G)]
    d_ranges, d_poses = dev(ranges), dev(poses1)
    rows = np.array([r for r, _ in KL_ROWS], np.int32).view(kl.REFRESH_ROW_DTYPE).reshape(-1)
    d_rows, d_res = dev(rows), dev(np.full((len(rows), 2), -77, np.int32))
    sync()
    f.refresh_device(len(rows), d_rows.data_ptr(), d_ranges.data_ptr(), d_poses.data_ptr(), KL_POOL, d_res.data_ptr())
    want_ref = {}
    for (g, first, _, pool_first), cnt in KL_ROWS:   # the twin: one host-indexed call per row
        if cnt and cnt > 0:
            twin.set_scans_device(g, first, cnt, d_ranges.data_ptr() + 8 * n * pool_first, d_poses.data_ptr() + 24 * pool_first)
            for j in range(cnt):
                want_ref[(g, first + j)] = pool_first + j
    got = [f.get_reference(g, 0, KL_N) for g in range(KL_G)]
    for g in range(KL_G):
        same(got[g], twin.get_reference(g, 0, KL_N), f"graph {g} against kl_set_scans_device")
    rest = LR.reference(laser_dict(n), bary, ranges, poses1)   # the restatement of every slot
    for (g, s), slot in want_ref.items():
        same(got[g][s], rest[slot], f"graph {g} scan {s} against the restatement")
    if bary:
        same(got[2][3], poses1[7, :2], "a scan without a valid reading: the sensor position")
    for g in range(KL_G):
        for s in range(KL_N):
            if (g, s) not in want_ref:
                same(got[g][s], before[g][s], f"graph {g} scan {s} is named by no row")
    assert all(k not in want_ref for k in KL_UNNAMED) and np.any(LR.bits(got[2][0]) != LR.bits(before[2][0]))
    want_res = [(r[3], c) if c is not None and c >= 0 else (0, 0) for r, c in KL_ROWS]
    assert host(d_res, np.int32, 2 * len(rows)).reshape(-1, 2).tolist() == [list(x) for x in want_res]
    assert f.refresh_info() == (4, kl.KL_EINVAL) and f.refresh_info() == (0, kl.KL_OK)
    with pytest.raises(Slam2dError) as e:
        f.refresh_device(4097, d_rows.data_ptr(), d_ranges.data_ptr(), d_poses.data_ptr(), KL_POOL)
    assert e.value.code == kl.KL_ERANGE
    f.close()
    twin.close()


def test_kl_refresh_refusals_are_ordered_by_call_then_row(gpu):
    """The first refusal is the minimum over (call, row), whatever order the workgroups ran in."""
    n = 8
    ranges, poses = pool_of(KL_POOL, n, 5)
    f = kl_fleet(n, 1)
    d_ranges, d_poses = dev(ranges), dev(poses)
    a = np.array([(2, 0, 1, 4), (2, 7, 2, 0), (9, 0, 1, 0)], np.int32)   # KL_ERANGE before KL_EINVAL
    b = np.array([(9, 0, 1, 0)], np.int32)
    d_a, d_b = dev(a), dev(b)
    sync()
    f.refresh_device(3, d_a.data_ptr(), d_ranges.data_ptr(), d_poses.data_ptr(), KL_POOL)
    f.refresh_device(1, d_b.data_ptr(), d_ranges.data_ptr(), d_poses.data_ptr(), KL_POOL)
    assert f.refresh_info() == (3, kl.KL_ERANGE)
    f.refresh_device(1, d_b.data_ptr(), d_ranges.data_ptr(), d_poses.data_ptr(), KL_POOL)
    assert f.refresh_info() == (1, kl.KL_EINVAL)
    f.close()


# ====================================================================================== 2. kt_refresh_device
KT_S = 8
KT_ROWS = [(0, 1), (3, 4), (5, 0), (-1, 2), (KT_S - 1, 2)]   # the last two are refused; slots 0 and 3 .. 6 are named
KT_NAMED = [0, 3, 4, 5, 6]


def matcher(n, loop=False):
    return kt.ScanMatcher(laser_of(n), kt.default_params(loop=loop), max_matches=1, max_scans=KT_S, max_base=3)


def kt_state(m):
    r, p, s = m.pool_device()
    n = m.laser.n_readings
    return peek(r, np.float64, (s, n)), peek(p, np.float64, (s, 3)), [m.prepared(k) for k in range(s)]


def same_prepared(a, b, what):
    assert a["npts"] == b["npts"], what
    for k in ("pts", "loc", "bad", "evt"):
        same(a[k], b[k], f"{what} {k}")


def match_bytes(m):
    """One kt_match_batch_device over refreshed scans: slot 3 against slots 4, 5, 6."""
    d_q, d_bb, d_bi = dev(np.array([3], np.int32)), dev(np.array([0, 3], np.int32)), dev(np.array([4, 5, 6], np.int32))
    d_out = dev(np.zeros(1, kt.RESULT_DTYPE))
    sync()
    m.match_batch_device(1, d_q.data_ptr(), d_bb.data_ptr(), d_bi.data_ptr(), d_out.data_ptr())
    sync()
    return host(d_out, np.uint8, kt.RESULT_DTYPE.itemsize)


@pytest.mark.parametrize("knob", KNOB, indirect=True)
@pytest.mark.parametrize("foreign", [False, True], ids=["in_place", "foreign"])
@pytest.mark.parametrize("n", READINGS + [4096])   # 4096: the scan's arrays and the prefix sum need more than 64 KB of LDS
def test_kt_refresh_equals_set_scans_device(knob, n, foreign):
    ranges0, poses0 = pool_of(KT_S, n, 300 + n, dead=4)
    ranges1, poses1 = pool_of(KT_S, n, 400 + n, dead=5)
    poses1[3:7] = poses1[3] + np.random.default_rng(n).normal(0.0, 0.02, (4, 3))   # the match's scans lie together
    m, twin = matcher(n), matcher(n)
    d_rows = dev(np.array(KT_ROWS, np.int32))
    for c in (m, twin):
        c.set_scans(0, ranges0, poses0)
    if foreign:
        d_r, d_p = dev(ranges1), dev(poses1)
        src = lambda c: (d_r.data_ptr(), d_p.data_ptr())   # noqa: E731
    else:   # the new readings and poses are already in the pool: the refresh is in place
        for c in (m, twin):
            r, p, _ = c.pool_device()
            poke(r, ranges1)
            poke(p, poses1)
        src = lambda c: c.pool_device()[:2]   # noqa: E731
    sync()
    m.refresh_device(len(KT_ROWS), d_rows.data_ptr(), *src(m), KT_S)
    for first, cnt in KT_ROWS[:3]:
        r, p = src(twin)
        twin.set_scans_device(first, cnt, r + 8 * n * first, p + 24 * first)
    got_r, got_p, got = kt_state(m)
    want_r, want_p, want = kt_state(twin)
    same(got_r, want_r, "pool ranges")
    same(got_p, want_p, "pool poses")
    for s in range(KT_S):
        same_prepared(got[s], want[s], f"slot {s}")
    old = matcher(n)   # what the first kt_set_scans alone leaves
    old.set_scans(0, ranges0, poses0)
    _, _, first_state = kt_state(old)
    old.close()
    for s in range(KT_S):
        if s in KT_NAMED:
            same(got_r[s], ranges1[s], f"slot {s} ranges")
            same(got_p[s], poses1[s], f"slot {s} pose")
        else:
            same_prepared(got[s], first_state[s], f"slot {s} is named by no row")
            if foreign:
                same(got_r[s], ranges0[s], f"slot {s} ranges")
                same(got_p[s], poses0[s], f"slot {s} pose")
    assert got[5]["npts"] == 0 and any(got[s]["npts"] > 0 for s in KT_NAMED)
    assert m.refresh_info() == (2, -1) and m.refresh_info() == (0, 0)
    same(match_bytes(m), match_bytes(twin), "kt_match_batch_device over the refreshed scans")
    with pytest.raises(Slam2dError) as e:
        m.refresh_device(4097, d_rows.data_ptr(), *src(m), KT_S)
    assert e.value.code == -5
    m.close()
    twin.close()


# ====================================================================================== 3. spa_compute_rows_device
def spa_cases():
    return [SR.case_ring(12, 2), SR.case_ring(33, 3), SR.case_hub(), SR.case_reversed(), SR.case_repeated()]


def spa_fleet(cases, extra=0):
    n = max(len(c["poses"]) for c in cases)
    m = max(len(c["ends"]) for c in cases)
    f = spa.SpaFleet(len(cases) + extra, n + 3, m + 5, n * (n + 1) // 2)
    for g, c in enumerate(cases):
        f.set_graph(g, c["ids"], c["poses"], c["ends"], c["means"], c["precs"])
    return f


def stats_bytes(f, g):
    st = spa.SpaStats()
    f._check(f.L.spa_get_stats(f.h, g, C.byref(st)), "spa_get_stats")
    return bytes(st)


@pytest.mark.parametrize("solver", ["pcg", "cholesky"])
def test_spa_compute_rows(gpu, solver):
    cases = spa_cases()
    f, twin = spa_fleet(cases), spa_fleet(cases)
    one = spa.default_params(solver=solver, niter=1)
    prm = spa.default_params(solver=solver)
    for c in (f, twin):   # one LM iteration each: every graph has stats, none is at its optimum
        c.compute(0, 5, one)
    start = [(f.get_nodes(g)[1], stats_bytes(f, g)) for g in range(5)]
    d_rows = dev(np.array([3, -1, 0, 3, 99], np.int32))
    sync()
    f.compute_rows_device(5, d_rows.data_ptr(), prm)
    twin.compute(3, 1, prm)
    twin.compute(0, 1, prm)
    for g in (3, 0):
        same(f.get_nodes(g)[1], twin.get_nodes(g)[1], f"graph {g} poses")
        assert stats_bytes(f, g) == stats_bytes(twin, g), g
        assert np.any(LR.bits(f.get_nodes(g)[1]) != LR.bits(start[g][0])), g
    for g in (1, 2, 4):
        same(f.get_nodes(g)[1], start[g][0], f"graph {g} is not computed")
        assert stats_bytes(f, g) == start[g][1], g
    assert f.rows_info() == (1, spa.SPA_EINVAL) and f.rows_info() == (0, 0)
    f.close()
    twin.close()


# ====================================================================================== 4. spa_export_poses_device
def test_spa_export_poses(gpu):
    rng = np.random.default_rng(8)
    P = 230
    perm = rng.permutation(65).astype(np.int32)
    dup = np.arange(65, dtype=np.int32)
    dup[10], dup[20] = 5, -1                       # node 10 has node 5's id and, coming later, wins; node 20 has none
    edge = np.arange(-1, 7, dtype=np.int32)        # ascending with an id of -1, and three slots beyond the pool
    ids = [np.zeros(0, np.int32), np.zeros(1, np.int32), np.arange(64, dtype=np.int32), perm, dup, edge]
    offsets = np.array([0, 3, 10, 80, 150, P - 4], np.int32)
    f = spa.SpaFleet(6, 70, 4)
    poses = []
    for g, i in enumerate(ids):
        po = rng.normal(0.0, 2.0, (len(i), 3))
        po[:, 2] = np.where(rng.random(len(i)) < 0.2, -0.0, po[:, 2])   # bits, not values
        poses.append(po)
        f.set_graph(g, i, po, np.zeros((0, 2), np.int32), np.zeros((0, 3)), np.zeros((0, 9)))
    assert np.all(np.diff(ids[2]) > 0) and np.all(np.diff(ids[5]) > 0) and not np.all(np.diff(perm) > 0)
    pool = np.frombuffer(bytes([0xA5]) * (P * 24), np.float64).reshape(P, 3).copy()
    want = pool.copy()
    skipped = 0
    for g, i in enumerate(ids):
        for k, id_ in enumerate(i.tolist()):
            slot = int(offsets[g]) + id_
            if id_ < 0 or slot >= P:
                skipped += 1
            else:
                want[slot] = poses[g][k]
    assert skipped == 5
    d_pool, d_off = dev(pool), dev(offsets)
    d_rows = dev(np.array([0, 1, 2, 3, 4, 5, -1, 7], np.int32))
    sync()
    f.export_poses_device(8, d_rows.data_ptr(), d_off.data_ptr(), d_pool.data_ptr(), P)
    got = host(d_pool, np.float64, P * 3).reshape(P, 3)
    same(got, want, "the pool")
    same(got[150 + 5], poses[4][10], "the later node of a duplicated id wins")
    untouched = np.ones(P, bool)
    for g, i in enumerate(ids):
        untouched[[offsets[g] + v for v in i.tolist() if v >= 0 and offsets[g] + v < P]] = False
    assert untouched.sum() > 20 and np.all(got[untouched].view(np.uint8) == 0xA5)
    # five skipped nodes and the row naming graph 7; the first in row order is row 4's node without an id
    assert f.rows_info() == (skipped + 1, spa.SPA_ERANGE) and f.rows_info() == (0, 0)
    f.close()


# ====================================================================================== 5. the stage
N_RING, POOL_FIRST = 40, 4
OFFSETS = (POOL_FIRST, POOL_FIRST + N_RING)
POOL = POOL_FIRST + 2 * N_RING + 4
S_NEW = N_RING - 1
RING_N = 8   # readings


class Fleet:
    """The contexts of one side: the loop-search fleet, the optimiser, the sequential and the loop matcher, and the
    scan pool.  Two 40-scan rings with drifted poses, so neither system is at its optimum."""

    def __init__(self):
        import torch

        lz = laser_of(RING_N)
        self.f = kl.LoopSearchFleet(lz, kl.default_params(link_scan_maximum_distance=1.5, loop_search_maximum_distance=4.0,
                                                         loop_match_minimum_chain_size=3, use_scan_barycenter=1),
                                    2, N_RING + 5, 200, 4)
        self.spa = spa.SpaFleet(2, N_RING + 5, 200)
        self.seq = kt.ScanMatcher(lz, kt.default_params(), max_matches=1, max_scans=POOL, max_base=3)
        self.loop = kt.ScanMatcher(lz, kt.default_params(loop=True), max_matches=1, max_scans=POOL, max_base=3)
        ranges, pool = pool_of(POOL, RING_N, 77)
        self.cases = [SR.case_ring(N_RING, 41 + g) for g in range(2)]
        for g, c in enumerate(self.cases):
            self.f.set_pool_offset(g, OFFSETS[g])
            self.f.set_graph(g, N_RING, [(i, i + 1) for i in range(N_RING - 1)])
            self.spa.set_graph(g, np.arange(N_RING, dtype=np.int32), c["poses"], c["ends"], c["means"], c["precs"])
            pool[OFFSETS[g]:OFFSETS[g] + N_RING] = c["poses"]
        self.d_ranges, self.d_pool = torch.from_numpy(ranges).cuda(), torch.from_numpy(pool).cuda()
        sync()
        for g in range(2):   # every scan's first refresh, host-indexed on both sides
            o = OFFSETS[g]
            self.f.set_scans_device(g, 0, N_RING, self.d_ranges[o:].data_ptr(), self.d_pool[o:].data_ptr())
        for m in (self.seq, self.loop):
            m.set_scans_device(0, POOL, self.d_ranges.data_ptr(), self.d_pool.data_ptr())
        sync()

    def state(self):
        out = {"pool": self.d_pool.cpu().numpy()}
        for g in range(2):
            out[f"ref{g}"] = self.f.get_reference(g, 0, N_RING)
            out[f"spa{g}"] = self.spa.get_nodes(g)[1]
        for name, m in (("seq", self.seq), ("loop", self.loop)):
            r, p, prepared = kt_state(m)
            out[f"{name}/ranges"], out[f"{name}/poses"] = r, p
            for s, d in enumerate(prepared):
                out[f"{name}/{s}/npts"] = np.array([d["npts"]])
                for k in ("pts", "loc", "bad", "evt"):
                    out[f"{name}/{s}/{k}"] = d[k]
        items = np.array([(g, S_NEW, 0, 12) for g in range(2)], np.int32)
        d_items, d_out = dev(items), dev(np.full((2, 2), -77, np.int32))
        sync()
        self.f.closest_device(2, d_items.data_ptr(), d_out.data_ptr())
        out["closest"] = host(d_out, np.int32, 4)
        return out

    def close(self):
        for c in (self.f, self.spa, self.seq, self.loop):
            c.close()


FINE_POSE = np.array([0.04, 0.02, -0.008])


def stage_records():
    jobs = ke.jobs([(g, S_NEW, OFFSETS[g], S_NEW - 1, g, -1, 0, 0) for g in range(2)])
    cl = np.zeros(2, ke.CLOSURE_DTYPE)
    cl["chain"], cl["resume"], cl["fine"] = [-1, 0], [-1, 30], [-1, 0]
    return jobs, cl


def run_stage(streams):
    """The fine pose write's refresh and CorrectPoses through kc_; streams: None (the contexts' own), or the streams
    the two calls alternate over."""
    import torch

    a = Fleet()
    stage = kc.PoseCorrection(2, N_RING + 5, OFFSETS, 8)
    for c in (stage, a.f, a.seq, a.loop):
        c.set_timing(True)
    jobs, cl = stage_records()
    d_jobs, d_cl = dev(jobs), dev(cl)
    a.d_pool[OFFSETS[1] + S_NEW] += torch.from_numpy(FINE_POSE).cuda()   # pScan->SetSensorPose(bestPose)
    sync()
    s = [0, 0] if streams is None else [x.cuda_stream for x in streams]
    stage.refresh_jobs_device(d_jobs.data_ptr(), d_cl.data_ptr(), 2, a.d_ranges.data_ptr(), a.d_pool.data_ptr(), POOL,
                              a.f, a.seq, a.loop, s[0])
    stage.correct_poses_device(d_jobs.data_ptr(), d_cl.data_ptr(), 2, a.spa, a.d_ranges.data_ptr(), a.d_pool.data_ptr(),
                               POOL, None, a.f, a.seq, a.loop, s[1])
    if streams is not None:
        streams[1].synchronize()   # the last call completed on its stream: nothing else is waited for
    info = stage.info()
    launches = {k: v[1] for c in (stage, a.f, a.seq, a.loop) for k, v in c.kernel_times().items() if v[1]}
    refusals = (a.f.refresh_info(), a.seq.refresh_info(), a.loop.refresh_info(), a.spa.rows_info())
    state = a.state()
    stage.close()
    a.close()
    return state, info, launches, refusals


def test_stage_equals_the_per_graph_loops(gpu):
    import torch

    got, info, launches, refusals = run_stage(None)
    # the twin: graph, first scan and count are host integers
    b = Fleet()
    start = b.state()
    b.d_pool[OFFSETS[1] + S_NEW] += torch.from_numpy(FINE_POSE).cuda()
    sync()
    o = OFFSETS[1] + S_NEW
    b.f.set_scans_device(1, S_NEW, 1, b.d_ranges[o:].data_ptr(), b.d_pool[o:].data_ptr())
    for m in (b.seq, b.loop):
        m.set_scans_device(o, 1, b.d_ranges[o:].data_ptr(), b.d_pool[o:].data_ptr())
    b.spa.compute(1, 1)
    d_poses, n = b.spa.device_poses(1)
    b.d_pool[OFFSETS[1]:OFFSETS[1] + n] = torch.from_numpy(peek(d_poses, np.float64, (n, 3))).cuda()   # CorrectPoses
    sync()
    o = OFFSETS[1]
    b.f.set_scans_device(1, 0, n, b.d_ranges[o:].data_ptr(), b.d_pool[o:].data_ptr())
    for m in (b.seq, b.loop):
        m.set_scans_device(o, n, b.d_ranges[o:].data_ptr(), b.d_pool[o:].data_ptr())
    want = b.state()
    assert set(got) == set(want)
    for k in want:
        same(got[k], want[k], k)
    # graph 1 moved, graph 0 did not: its poses, references and prepared scans are the first refresh's
    assert np.any(LR.bits(want["spa1"]) != LR.bits(start["spa1"])) and np.any(LR.bits(want["ref1"]) != LR.bits(start["ref1"]))
    for k in ("spa0", "ref0"):
        same(got[k], start[k], k)
    same(got["pool"][:OFFSETS[1]], start["pool"][:OFFSETS[1]], "graph 0's pool poses")
    for s in range(OFFSETS[1]):
        same(got[f"seq/{s}/pts"], start[f"seq/{s}/pts"], f"slot {s}")
    # ... although its system is not at its optimum: on the twin alone, a compute of graph 0 moves it
    b.spa.compute(0, 1)
    assert np.any(LR.bits(b.spa.get_nodes(0)[1]) != LR.bits(start["spa0"]))
    b.close()
    assert info == (1, 1, 0)   # one scan named by the refresh call's records, one graph corrected, nothing refused
    assert refusals == ((0, 0),) * 4
    # per call one flatten and one kernel per context (the optimiser's two kernels are not timed)
    assert launches == {"kc_flatten_kernel": 2, "kl_refresh_kernel": 2, "kt_refresh_kernel": 2}


def test_stage_on_caller_streams(gpu):
    """The same sequence on one caller's stream and on two alternating streams gives the same bytes."""
    import torch

    want = run_stage(None)[0]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for streams in ((s1, s1), (s1, s2)):
        got = run_stage(streams)[0]
        for k in want:
            same(got[k], want[k], k)


# ====================================================================================== 6. kc_refresh_intake_device
def test_refresh_intake_names_only_the_accepted_scan(gpu, monkeypatch):
    monkeypatch.setenv("SLAM2D_POISON", "1")
    G, N, n = 4, 8, RING_N
    lz = laser_of(n)
    prm = kl.default_params(use_scan_barycenter=1)
    ranges, poses0 = pool_of(G * N, n, 21)
    _, poses1 = pool_of(G * N, n, 22)

    def side():
        f = kl.LoopSearchFleet(lz, prm, G, N, 4, 1)
        m = kt.ScanMatcher(lz, kt.default_params(), max_matches=1, max_scans=G * N, max_base=1)
        for g in range(1, G):
            f.add_vertex(g)
        for g in range(G):
            f.set_scans(g, 0, ranges[g * N:g * N + 1], poses0[g * N:g * N + 1])
        m.set_scans(0, ranges, poses0)
        return f, m

    f, m = side()
    tf, tm = side()
    sp = spa.SpaFleet(G, N, 4)
    rec = np.zeros(5, kp.INTAKE_DTYPE)
    rec["scan"], rec["prev"] = -1, -1
    rec[0]["accepted"], rec[0]["scan"] = 1, 0                                  # accepted: graph 0's first scan
    rec[0]["corrected"] = poses1[0]
    rec[1]["corrected"] = poses1[N]                                            # rejected: its poses, accepted 0
    rec[3]["status"], rec[3]["accepted"], rec[3]["scan"] = kp.KP_ERANGE, 1, 0  # a status other than KP_OK
    rec[4]["accepted"], rec[4]["scan"] = 1, N + 1                              # (a fifth record, used alone below)
    d_rec = dev(rec)
    edits, stage = kd.GraphEdits(8), kc.PoseCorrection(G, N, None, 8)
    d_ranges, d_poses = dev(ranges), dev(poses1)
    sync()
    edits.commit_vertices_device(d_rec.data_ptr(), 0, 4, f, sp)    # graph 0 is edited on the device
    stage.refresh_intake_device(d_rec.data_ptr(), 0, 4, d_ranges.data_ptr(), d_poses.data_ptr(), G * N, f, m, None)
    assert stage.info() == (1, 0, 0)
    tf.set_scans_device(0, 0, 1, d_ranges.data_ptr(), d_poses.data_ptr())
    tm.set_scans_device(0, 1, d_ranges.data_ptr(), d_poses.data_ptr())
    rest = LR.reference(laser_dict(n), 1, ranges[:1], poses1[:1])
    for g in range(G):
        same(f.get_reference(g, 0, N), tf.get_reference(g, 0, N), f"graph {g}")
    same(f.get_reference(0, 0, 1), rest, "the accepted scan against the restatement")
    for a, b in zip(kt_state(m)[2], kt_state(tm)[2]):
        same_prepared(a, b, "prepared")
    same(kt_state(m)[1], kt_state(tm)[1], "pool poses")
    # the refresh did not need the host's copy of the graph: the counts are still pulled back afterwards
    assert edits.info() == (1, 0, 0)
    assert f.counts(0) == (1, 0) and sp.counts(0) == (1, 0) and f.counts(1) == (1, 0) and sp.counts(1) == (0, 0)
    # a record whose scan lies outside [0, max_scans) is refused by the stage and reaches no context
    before = f.get_reference(0, 0, N)
    stage.refresh_intake_device(d_rec.data_ptr() + 4 * kp.INTAKE_DTYPE.itemsize, 0, 1, d_ranges.data_ptr(),
                                d_poses.data_ptr(), G * N, f, m, None)
    assert stage.info() == (0, 0, 1) and f.refresh_info() == (0, 0) and m.refresh_info() == (0, 0)
    same(f.get_reference(0, 0, N), before, "graph 0")
    for c in (f, m, tf, tm, sp, edits, stage):
        c.close()
