"""Directed inputs of the Hector matcher tests -- TEST INFRASTRUCTURE ONLY.

tests/test_hector_match_gpu.py runs every case through hs_match_kernel and through the CPU oracle;
tests/test_hector_match_cpu.py holds the oracle to the plain statement (hector_match_plain.py) on a subset, and
runs test_case_preconditions (below), which asserts with the oracle alone that each case reaches the path it is
named after.  Maps are built once per geometry: a few synthetic scans through the oracle's own grid update, then
hand-built edits; both sides of a comparison load them (HectorFleet.set_map / HectorOracle.set_level), so no update
kernel takes part.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import oracle as O
from slam2d import synth

import hector_match_plain as P


@dataclass(frozen=True)
class Geo:
    res: float
    sx: int
    sy: int
    start: tuple
    levels: int

    def oracle(self, reduce_threads=0):
        return O.HectorOracle(self.res, self.sx, self.start, self.levels, reduce_threads=reduce_threads,
                              map_size_y=self.sy)

    def pyramid(self):
        return P.pyramid(self.res, self.sx, self.sy, self.start, self.levels)

    def with_levels(self, levels):
        return Geo(self.res, self.sx, self.sy, self.start, levels)


@dataclass(frozen=True)
class Case:
    name: str
    geo: Geo
    pts: np.ndarray          # float32 [n, 2], level-0 cells
    hint: tuple              # world pose
    origo: tuple = (0.0, 0.0)
    expect: str = ""         # the path test_case_preconditions asserts
    edits: bool = False      # the map with the hand-built cells

    @property
    def n(self):
        return int(self.pts.shape[0])


# ------------------------------------------------------------------------------------------------ scans and maps
@functools.lru_cache(maxsize=None)
def _stream(res, n_beams, seed):
    return synth.make_streams(1, 6, seed=seed, n_beams=n_beams, scale_to_map=float(np.float32(1.0) / np.float32(res)))


def scan(res, n, k=5, seed=4242):
    """n points of synthetic scan k (evenly thinned from a scan of enough beams), in cells of resolution res."""
    n_beams = 1081 if n <= 900 else 2881
    S = _stream(res, n_beams, seed)
    m = int(S.counts[0, k])
    assert n <= m, (n, m)
    idx = np.unique(np.linspace(0, m - 1, n).round().astype(np.int64)) if n else np.zeros(0, np.int64)
    assert idx.size == n
    return np.ascontiguousarray(S.points[0, k, idx], np.float32)


# the hand-built cells (x, y, log-odds): saturated, beyond the occupied clamp (50 + lo), far below, and exact zeros,
# around the tile seam (64, 32), 4-cell block seams and the map limits of a 96 x 80 level
LO = float(np.float32(np.log(np.float32(0.9) / (np.float32(1.0) - np.float32(0.9)))))
EDIT_VALUES = (0.0, 50.0, -50.0, 50.0 + LO, -200.0, 80.0)


def _edit(l, lvl):
    """(the values rotate from level to level, so that cell (0, 0) and its neighbours differ between levels)"""
    sy, sx = l.shape
    spots = [(63, 31), (64, 31), (63, 32), (64, 32), (65, 33), (62, 30), (3, 3), (4, 4), (4, 3), (3, 4), (7, 8), (8, 7),
             (0, 0), (1, 0), (0, 1), (1, 1), (sx - 2, 5), (sx - 1, 5), (sx - 2, 6), (sx - 1, 6), (sx - 3, 5), (sx - 3, 6),
             (10, sy - 2), (10, sy - 1), (11, sy - 2), (11, sy - 1)]
    k = 1 + lvl
    for (x, y) in spots:
        if 0 <= x < sx and 0 <= y < sy:
            l[y, x] = EDIT_VALUES[k % len(EDIT_VALUES)]
            k += 1
    return l


@functools.lru_cache(maxsize=None)
def maps(geo: Geo, edits=False, n_scans=4):
    """Per level (log-odds [sy, sx] float32, updateIndex int32) after n_scans synthetic scans (forced updates).  The
    updateIndex planes are handed out as -1 (never updated): the maps are loaded into fresh streams whose update index
    starts at 0, and cells marked ahead of their map's own index are a state neither the reference nor the library
    produces (the grid update of the batched case's first step would treat them differently on the two sides)."""
    ora = geo.oracle()
    ora.set_update_factors(0.4, 0.9)
    ora.set_thresholds(-1.0, -1.0)
    S = _stream(geo.res, 1081, 4242)
    for k in range(n_scans):
        ora.process(S.points[0, k, : S.counts[0, k]])
    out = []
    for lvl in range(geo.levels):
        l, u = ora.level(lvl)
        l = l.copy()
        if edits:
            _edit(l, lvl)
        u = np.full_like(u, -1)
        l.setflags(write=False)
        u.setflags(write=False)
        out.append((l, u))
    ora.close()
    return tuple(out)


def load(target, geo, edits=False, stream=None):
    """Load the geometry's maps into a HectorOracle, or into one stream of a HectorFleet."""
    for lvl, (l, u) in enumerate(maps(geo, edits)):
        if stream is None:
            target.set_level(lvl, l, u)
        else:
            target.set_map(stream, lvl, l, u)


def run_oracle(case: Case, reduce_threads=0, trace=False):
    """(pose, cov, clamp count, trace or None) of the case in the oracle."""
    ora = case.geo.oracle(reduce_threads)
    load(ora, case.geo, case.edits)
    if trace:
        ora.enable_trace(64)
    pose, cov = ora.match(case.pts, np.asarray(case.hint, np.float32), case.origo)
    out = (pose, cov, ora.clamp_count(), ora.trace() if trace else None)
    ora.close()
    return out


# ------------------------------------------------------------------------------------------------ the case families
G256 = Geo(0.1, 256, 256, (0.5, 0.5), 2)         # 25.6 m square
G96 = Geo(0.25, 96, 80, (0.01, 0.5), 3)          # 96 x 80, 48 x 40, 24 x 20: padded 64 x 32 tiles at every level
G128 = Geo(0.25, 128, 128, (0.5, 0.5), 2)        # the batched launch's maps
GNAN = Geo(0.05, 256, 256, (0.5, 0.5), 2)

# 1. every chunk tail of the chain wave's unrolled sum (192 points per chunk), waves straddling n, the chunk and
#    register-slot boundaries up to CW_MAXN = 1152
COUNTS_1152 = tuple(range(1, 401)) + (575, 576, 577, 768, 769, 960, 961, 1151, 1152)
# 2. (max_points, reduction order, counts): the other instantiations of hs_match_kernel.  hs_match refuses n > max_points,
#    so the counts beyond 1153 / 1281 run on instances of the same kind with room for them (2000 / 1537)
OTHER_INSTANCES = (
    (1153, 0, (1, 192, 1152, 1153)),                  # SEQ, not REGS: gn_step_cw up to 1152, the HBM gn_step at 1153
    (2000, 0, (1152, 1153, 1281, 1409, 2000)),        # the same instance: the HBM gn_step and its split gathers
    (1280, 256, (1, 255, 256, 257, 1279, 1280)),      # tree order, REGS
    (1281, 256, (1280, 1281)),                        # tree order, not REGS
    (1537, 256, (1280, 1281, 1537)),
)

HINT_TRUE = (0.3, 0.0115, 0.0955)   # where scan 5 matches the map of scans 0 .. 3 (the 4-level match from any near hint)
# hints from which points leave the level-0 map during the iterations and come back, by (n, levels): found by a
# search with the oracle, pinned by test_case_preconditions
LEAVE_RETURN = {(300, 1): (2.2, -0.22, 0.0), (300, 2): (2.53, 0.74, -0.29), (300, 3): (-0.68, -0.8, 0.1),
                (300, 4): (-1.68, 0.82, 0.13), (1000, 1): (-1.96, -0.22, 0.18), (1000, 2): (3.19, 0.3, -0.16),
                (1000, 3): (2.82, 0.98, 0.13), (1000, 4): (-2.23, 0.46, -0.05)}


def hint_cases():
    """Family 3: hints, at n = 300 and 1000, 1 to 4 levels of a 256^2 map."""
    out = []
    far = 1.0e6
    # every point off the map: the scan moved 10^5 cells away under a hint that the world -> map -> world round trip of
    # every level returns exactly (the returned pose is that round trip: ScanMatcher.h:96), or a hint 10^6 m away
    away = (0.5, 0.25, 0.4)
    hints = [("exact", HINT_TRUE, ""), ("small", (0.03, -0.02, 0.015), ""), ("far", (0.3, 0.2, 0.3), ""),
             ("rot08", (0.0, 0.0, 0.8), ""), ("leave_return", None, "leave_return"),
             ("heading_p31", (0.0, 0.0, 3.1), ""), ("heading_m31", (0.0, 0.0, -3.1), ""),
             ("heading_wrap_p", (0.05, 0.0, 3.3), "wrap"), ("heading_wrap_m", (0.0, 0.05, -3.4), "wrap"),
             ("heading_2pi", (0.0, 0.0, 6.3), "wrap"), ("all_out", away, "all_out"),
             ("all_out_far", (far, -far, 0.4), "all_out_far"),
             ("nan_x", (np.nan, 0.0, 0.0), "nan"), ("nan_theta", (0.0, 0.0, np.nan), "nan")]
    for levels in (1, 2, 3, 4):
        geo = G256.with_levels(levels)
        for n in (300, 1000):
            for name, hint, expect in hints:
                h = LEAVE_RETURN[(n, levels)] if hint is None else hint
                pts = scan(geo.res, n) + np.float32(1.0e5 if name == "all_out" else 0.0)
                out.append(Case(f"{name}_n{n}_l{levels}", geo, pts, h, expect=expect))
    return out


def nan_cases():
    """On the 12.8 m map (mostly free space: few cells carry a gradient) a hint rotated by 0.3 rad makes H singular
    with a non-zero diagonal at 300 points: the pose turns NaN in mid-match.  At 600 / 900 points the same hint
    is cut at 0.2 rad and the pose runs tens of metres off the map, staying finite."""
    g1 = GNAN.with_levels(1)
    return [Case("singular_H", g1, scan(GNAN.res, 300), (0.0, 0.0, 0.3), expect="nan_mid"),
            Case("runaway_n600_l1", g1, scan(GNAN.res, 600), (0.0, 0.0, 0.3), expect="clamp"),
            Case("runaway_n600_l2", GNAN, scan(GNAN.res, 600), (0.0, 0.0, 0.3), expect="clamp"),
            Case("runaway_n900_l1", g1, scan(GNAN.res, 900), (0.0, 0.0, 0.3), expect="clamp")]


CLAMP_PLUS_IDX, CLAMP_PLUS_HINT = (5, 8, 89, 117, 123, 129, 167, 174, 193), (-0.11, 0.3, -0.11)
CLAMP_MINUS_IDX, CLAMP_MINUS_HINT = (6, 32, 36, 64, 89, 107, 114, 128, 152, 154, 184), (0.59, -0.16, 0.3)


def clamp_cases():
    """A dozen points on the 96 x 80 map whose rotation update exceeds 0.2 rad in a step with cond(H) <= 1e5 (so the
    CPU test can judge the decision): one cut at +0.2, one at -0.2; both still settle on the scan's pose.  Found by a
    search with the oracle; pinned by test_case_preconditions."""
    geo = G96.with_levels(1)
    base = scan(geo.res, 200)
    return [Case("clamp_plus", geo, base[list(CLAMP_PLUS_IDX)], CLAMP_PLUS_HINT, expect="clamp+", edits=True),
            Case("clamp_minus", geo, base[list(CLAMP_MINUS_IDX)], CLAMP_MINUS_HINT, expect="clamp-", edits=True)]


def _first_pose(geo, hint):
    """The map-frame pose of the first step (coarsest level), as the oracle computes it."""
    ora = geo.oracle()
    ora.enable_trace(4)
    far = np.array([[1.0e7, 1.0e7]], np.float32)
    ora.match(far, np.asarray(hint, np.float32))
    p = ora.trace()[0, :3].copy()
    ora.close()
    return p


def geometry_cases():
    """Family 4: the 96 x 80 map (map_start (0.01, 0.5), origo != 0) with hand-built cells; points landing exactly on
    x = 0, on the limits x = sx - 2 / y = sy - 2 (inside), just beyond them (outside), on both sides of the tile seam
    (64, 32) and of 4-cell block seams, in the first step of the coarsest level (heading 0: the rotation is exact)."""
    out = []
    for levels in (1, 3):
        geo = G96.with_levels(levels)
        top = geo.pyramid()[-1]
        # a hint whose first map pose has integer coordinates: map_start 0.01 puts the world origin at 0.24 m, so the
        # float32 neighbours of 2 cells - 0.24 m are tried until the oracle's own first pose is the integer
        hint = est = None
        w0 = np.float32(2.0 * top.cell_len - 0.24)
        for k in range(-16, 17):
            wx = w0
            for _ in range(abs(k)):
                wx = np.nextafter(wx, np.float32(np.inf if k > 0 else -np.inf))
            e = _first_pose(geo, (float(wx), -1.0, 0.0))
            if e[0] == 2.0 and e[1] == np.round(e[1]):
                hint, est = (float(wx), -1.0, 0.0), e
                break
        assert hint is not None
        lim_x, lim_y = top.sx - 2.0, top.sy - 2.0
        up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))      # noqa: E731
        dn = lambda v: float(np.nextafter(np.float32(v), np.float32(-np.inf)))     # noqa: E731
        below0 = float(np.float32(2.0) + np.nextafter(np.float32(-2.0), np.float32(-np.inf)))   # the last sum below 0
        tgt = [(0.0, 5.5), (below0, 5.5), (lim_x, 5.25), (up(lim_x), 5.25), (dn(lim_x), 5.75), (10.5, lim_y),
               (10.5, up(lim_y)), (10.25, 0.0), (lim_x, lim_y), (0.0, 0.0), (3.5, 3.5), (4.0, 4.0), (dn(4.0), dn(4.0)),
               (7.75, 8.0), (8.0, 7.25), (4.5, 3.75)]
        if levels == 1:
            tgt += [(63.5, 31.5), (64.5, 31.5), (63.5, 32.5), (64.5, 32.5), (dn(64.0), dn(32.0)), (64.0, 32.0),
                    (63.25, 30.5), (65.5, 33.5), (dn(64.0), 5.0), (64.0, 5.0), (20.0, dn(32.0)), (20.0, 32.0)]
        tgt = np.asarray(tgt, np.float64)
        pts = ((tgt - est[None, :2].astype(np.float64)) / top.f).astype(np.float32)
        body = scan(geo.res, 150)
        for name, extra in (("directed", np.zeros((0, 2), np.float32)), ("directed_scan", body)):
            out.append(Case(f"geo_{name}_l{levels}", geo, np.concatenate([pts, extra]), hint, origo=(1.5, -0.75),
                            expect="landing", edits=True))
        out.append(Case(f"geo_rot_l{levels}", geo, np.concatenate([pts, body]), (2.1, -0.9, 0.35), origo=(1.5, -0.75),
                        edits=True))
        out.append(Case(f"geo_scan_l{levels}", geo, scan(geo.res, 400), (0.1, 0.05, -0.05), origo=(-2.0, 3.0), edits=True))
    return out


def _same_cell_points(case: Case, trace):
    """For every level l >= 1: a level-0-scale point that lies in cell (0, 0) of level l in that level's last step and
    in cell (0, 0) of level l - 1 in its first step.  The last step moves the point by delta cells (measured on the
    case's current points), so it is placed at a on level l with a and 2 (a + delta) both well inside (0, 1)."""
    pyr = case.geo.pyramid()
    out, row = [], 0
    for j, lvl in enumerate(range(case.geo.levels - 1, 0, -1)):
        row += 4
        cur = case.pts[case.n - (case.geo.levels - 1) + j][None, :]
        xa, ya, _ = scan_in_map_f64(pyr[lvl], trace[row - 1, :3], cur)
        xb, yb, _ = scan_in_map_f64(pyr[lvl - 1], trace[row, :3], cur)
        tgt = []
        for va, vb in ((xa[0], xb[0]), (ya[0], yb[0])):
            delta = vb / 2.0 - va
            lo, hi = max(0.05, 0.025 - delta), min(0.95, 0.475 - delta)
            tgt.append(0.5 * (lo + hi))   # (lo < hi whenever the last step moves the point by less than 0.4 cell:
            #                                test_case_preconditions asserts where the point ends up)
        x, y, th = (float(v) for v in trace[row - 1, :3])
        c, s = np.cos(th), np.sin(th)
        dx, dy = tgt[0] - x, tgt[1] - y
        out.append(((c * dx + s * dy) * 2.0 ** lvl, (-s * dx + c * dy) * 2.0 ** lvl))
    return np.asarray(out, np.float32)


def scan_in_map_f64(L, pose, pts):
    return P.scan_in_map(L, np.asarray(pose, np.float64), pts)


def same_cell_cases():
    """A point whose neighbourhood is cell (0, 0) at the end of one level and at the start of the next finer one (the
    only cell two levels can share: coordinates double from level to level).  Its cache key is then the same on both
    levels while the cells differ: the matcher has to forget its cached neighbourhoods between levels.  The
    points follow from the oracle's own trajectory (a few rounds: they move it slightly)."""
    out = []
    for levels in (2, 3):
        geo = G96.with_levels(levels)
        body, hint = scan(geo.res, 400), (0.1, 0.05, -0.05)
        extra = np.zeros((levels - 1, 2), np.float32)
        for _ in range(8):
            case = Case(f"same_cell_l{levels}", geo, np.concatenate([body, extra]), hint, origo=(0.5, 0.5),
                        expect="same_cell", edits=True)
            nxt = _same_cell_points(case, run_oracle(case, trace=True)[3])
            if np.abs(nxt - extra).max() < 1.0e-3:
                break
            extra = nxt
        out.append(case)
    return out


def batch_cases(B=264, seed=99):
    """Family 5: one batched launch over B streams on equal 128^2 maps; stream s has its own count (from COUNTS_1152)
    and its own hint.  Two steps: [0] the first scan (always drawn into the map, by both sides), [1] the scan under
    test.  Returns (counts [2, B], points [2, B, 1152, 2], hints [2, B, 3])."""
    rng = np.random.default_rng(seed)
    counts = np.empty((2, B), np.int32)
    counts[0] = rng.choice(np.asarray(COUNTS_1152), B)
    counts[1] = rng.choice(np.asarray(COUNTS_1152), B)
    counts[1, :12] = (1, 191, 192, 193, 383, 384, 385, 576, 577, 1151, 1152, 64)
    counts[1, 256:264] = (1152, 1, 193, 400, 960, 961, 7, 65)        # block ids with a non-zero b >> 8
    pts = np.zeros((2, B, 1152, 2), np.float32)
    hints = np.zeros((2, B, 3), np.float32)
    for t in range(2):
        for s in range(B):
            pts[t, s, : counts[t, s]] = scan(G128.res, int(counts[t, s]), k=4 + t)
        hints[t] = rng.uniform(-1.0, 1.0, (B, 3)) * np.array([0.15, 0.15, 0.1])
    return counts, pts, hints


# ------------------------------------------------------------------------------------------------ preconditions
def inside_counts(case: Case, trace):
    """Per step of the trace, which points lie inside their level's map (plain float64 evaluation)."""
    pyr = case.geo.pyramid()
    out = []
    i = 0
    for lvl in range(case.geo.levels - 1, -1, -1):
        for _ in range(6 if lvl == 0 else 4):
            x, y, _p = P.scan_in_map(pyr[lvl], trace[i, :3], case.pts)
            with np.errstate(invalid="ignore"):
                out.append((x >= 0) & (x <= pyr[lvl].sx - 2) & (y >= 0) & (y <= pyr[lvl].sy - 2))
            i += 1
    return np.asarray(out)


def check_precondition(case: Case):
    pose, cov, clamps, tr = run_oracle(case, trace=True)
    H = tr[:, 3:12]
    if case.expect == "all_out_far":
        assert not H.any() and clamps == 0     # (the pose is the hint's round trip through the coarsest map frame)
    elif case.expect == "all_out":
        assert not H.any() and clamps == 0
        assert np.array_equal(pose.view(np.int32), np.asarray(case.hint, np.float32).view(np.int32)), (pose, case.hint)
    elif case.expect == "nan":
        assert np.isnan(pose).any() and clamps == 0
    elif case.expect == "nan_mid":
        assert np.isfinite(tr[0, :3]).all() and np.isfinite(tr[1, :3]).all(), "the first steps are finite"
        assert np.isnan(pose).any(), pose
        k = int(np.flatnonzero(~np.isfinite(tr[:, :3]).all(axis=1))[0])   # the first step starting from a NaN pose
        assert H[k - 1, 0] != 0.0 and H[k - 1, 4] != 0.0, "the step before it had a non-zero diagonal"
    elif case.expect == "wrap":
        assert abs(case.hint[2]) > np.pi and abs(pose[2]) <= np.pi and np.isfinite(pose).all(), pose
    elif case.expect == "leave_return":
        ins = inside_counts(case, tr)
        lvl0 = ins[-6:]
        gone = lvl0[0][None, :] & ~lvl0[1:-1]                     # inside at first, outside at some later step
        back = np.zeros(lvl0.shape[1], bool)
        for j in range(gone.shape[0]):
            back |= gone[j] & lvl0[j + 2:].any(axis=0)
        assert back.sum() >= 3, f"{case.name}: {back.sum()} points leave the map and return"
    elif case.expect in ("clamp", "clamp+", "clamp-"):
        assert clamps >= 1 and np.isfinite(pose).all(), (case.name, clamps, pose)
    elif case.expect == "same_cell":
        pyr, maps_ = case.geo.pyramid(), maps(case.geo, case.edits)
        row = 0
        for j, lvl in enumerate(range(case.geo.levels - 1, 0, -1)):
            row += 4
            p = case.pts[case.n - (case.geo.levels - 1) + j][None, :]
            for L, r in ((pyr[lvl], row - 1), (pyr[lvl - 1], row)):     # the level's last step, the next level's first
                x, y, _p = P.scan_in_map(L, tr[r, :3], p, np.float32)
                assert 0.05 < x[0] < 0.95 and 0.05 < y[0] < 0.95, (case.name, lvl, r, x, y)
            a, b = maps_[lvl][0][:2, :2], maps_[lvl - 1][0][:2, :2]
            assert (P.occupancy(a) != P.occupancy(b)).any(), "the shared cell's neighbourhood differs between the levels"
    elif case.expect == "landing":
        top = case.geo.pyramid()[-1]
        est = tr[0, :3]
        assert est[2] == 0.0 and est[0] == np.round(est[0]) and est[1] == np.round(est[1]), est
        p32 = case.pts * np.float32(top.f)
        x = est[0] + p32[:, 0]      # float32, as any float32 evaluation at heading 0 (cos = 1, sin = 0)
        y = est[1] + p32[:, 1]
        lx, ly = np.float32(top.sx - 2), np.float32(top.sy - 2)
        assert np.any(x == 0.0) and np.any(x == lx) and np.any(y == ly) and np.any(y == 0.0)
        assert np.any(x == np.nextafter(lx, np.float32(np.inf))) and np.any(y == np.nextafter(ly, np.float32(np.inf)))
        assert np.any((x < 0.0) & (x > -1.0e-6))
        if top.sx > 65:
            assert np.any((x >= 63) & (x < 64) & (y >= 31) & (y < 32)) and np.any((x >= 64) & (y >= 32))
            assert np.any(x == np.nextafter(np.float32(64), np.float32(0))) and np.any(x == 64.0)
        assert H[0].any(), "the directed points see a gradient"
    return pose, cov, clamps, tr


def all_directed_cases():
    return hint_cases() + nan_cases() + clamp_cases() + geometry_cases() + same_cell_cases()


def test_case_preconditions():
    """Every directed case reaches the path it is named after (asserted with the oracle alone)."""
    seen = set()
    for case in all_directed_cases():
        if case.expect:
            check_precondition(case)
            seen.add(case.expect)
    assert seen >= {"all_out", "nan", "nan_mid", "wrap", "leave_return", "clamp", "clamp+", "clamp-", "landing", "same_cell"}, seen
    # the clamp signs: the rotation of the clamped step is exactly +-float32(0.2)
    for case, sign in zip(clamp_cases(), (1.0, -1.0)):
        _, _, clamps, tr = run_oracle(case, trace=True)
        d = tr[1:, 2].astype(np.float64) - tr[:-1, 2].astype(np.float64)
        assert np.any(np.abs(d - sign * float(np.float32(0.2))) <= 2.0 ** -22), (case.name, d)
