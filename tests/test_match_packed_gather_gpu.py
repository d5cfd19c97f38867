"""Directed cases of the packed gather of hs_match_kernel's reference-order register instance (gn_step_cw), against
the CPU oracle bit for bit.

On every Gauss-Newton step but a level's first, a point wave lists the points whose cell changed (its misses), parks
each one's key in the slot's plane-0 word and gathers the listed neighbourhoods packed, 64 list entries per pass.
The cases place the misses where that pass can go wrong: none at all, one in lane 0 or lane 63, every lane of every
slot (six full passes), 65 and 63 in one wave (a partial last pass), the point counts around a wave, a chunk and the
register-slot limit, points leaving and re-entering the map between steps, missed neighbourhoods across block and
tile seams of hand-built cells, many lanes missing one cell, three levels, and one ragged batched launch with every
chain wave.

Which points miss on which step is worked out here from the oracle's own trajectory (its trace holds every step's
starting pose): point i of a scan sits in slot i of its stream; slot = j * 192 + pt, point thread pt = 64 * wave +
lane.  A case asserts the miss pattern it is named after before it compares, with every point it relies on at least
MARGIN away from a cell border (float32 and float64 then agree on its cell).  Cases come from
tests/ref/hector_match_cases.py where it has them.
"""
import os
import sys

import numpy as np
import pytest

from slam2d.hector import HectorFleet

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import hector_match_cases as K  # noqa: E402
import hector_match_plain as P  # noqa: E402

pytestmark = pytest.mark.gpu

CW_PTS = 192      # point threads of a workgroup (three waves)
MARGIN = 2.0e-3   # cells: float32 map coordinates below 256 carry errors of a few 1e-5
G1 = K.G256.with_levels(1)
G96_1 = K.G96.with_levels(1)


def _same_bits(got, want, what):
    g = np.ascontiguousarray(got, np.float32).ravel()
    w = np.ascontiguousarray(want, np.float32).ravel()
    ok = (g.view(np.int32) == w.view(np.int32)) | (np.isnan(g) & np.isnan(w))
    assert ok.all(), f"{what}: kernel {g} ({g.view(np.int32)}) oracle {w} ({w.view(np.int32)})"


# ------------------------------------------------------------------------------- the oracle's trajectory and its misses
def trace_of(geo, edits, pts, hint):
    """The oracle's trace of the match: one row per Gauss-Newton step, [:3] the pose the step starts from."""
    ora = geo.oracle()
    K.load(ora, geo, edits)
    ora.enable_trace(64)
    ora.match(pts, np.asarray(hint, np.float32))
    tr = ora.trace()
    ora.close()
    return tr


def steps_of(geo):
    """(level, first) per trace row."""
    out = []
    for lvl in range(geo.levels - 1, -1, -1):
        for it in range(6 if lvl == 0 else 4):
            out.append((lvl, it == 0))
    return out


def cells_of(geo, tr, pts):
    """Per step: cell x, cell y (-1: outside the map), and the distance of the point to the nearest cell border or
    map limit [steps, n], in float64."""
    pyr = geo.pyramid()
    cx, cy, mg = [], [], []
    for row, (lvl, _) in enumerate(steps_of(geo)):
        L = pyr[lvl]
        with np.errstate(invalid="ignore"):
            x, y, _p = P.scan_in_map(L, tr[row, :3], pts)
            inside = (x >= 0) & (x <= L.sx - 2) & (y >= 0) & (y <= L.sy - 2)
            m = np.minimum(np.abs(x - np.round(x)), np.abs(y - np.round(y)))
        cx.append(np.where(inside, np.floor(x), -1))
        cy.append(np.where(inside, np.floor(y), -1))
        mg.append(np.where(np.isfinite(m), m, 1.0))
    return np.asarray(cx), np.asarray(cy), np.asarray(mg)


def misses_of(geo, tr, pts):
    """miss[step, i]: point i gathers on that step -- it is inside the map and its cell is not the one it gathered
    last (a point that left the map keeps its cached cell); packed[step]: the step is not a level's first."""
    cx, cy, mg = cells_of(geo, tr, pts)
    st = steps_of(geo)
    miss = np.zeros(cx.shape, bool)
    key = None
    for row, (lvl, first) in enumerate(st):
        k = cx[row] + 65536.0 * cy[row]
        if first:
            key = np.full(cx.shape[1], -2.0)
        ins = cx[row] >= 0
        miss[row] = ins & (k != key)
        key = np.where(miss[row], k, key)
    return miss, np.asarray([not f for _, f in st]), mg


def wave_of(i):
    return (np.asarray(i) % CW_PTS) // 64


def lane_of(i):
    return np.asarray(i) % 64


# ------------------------------------------------------------------------------------------------------ placed cases
def _to_scan(L, pose, xy):
    """The level-0-scale scan points that the pose puts at the map coordinates xy."""
    x, y, th = (float(v) for v in pose)
    c, s = np.cos(th), np.sin(th)
    dx, dy = xy[:, 0] - x, xy[:, 1] - y
    return (np.stack([c * dx + s * dy, -s * dx + c * dy], 1) / L.f).astype(np.float32)


def centred(geo, edits, pts, hint):
    """pts moved (by less than a cell each) to the centres of the cells the first step finds them in; the first
    step's pose is the hint's, whatever the points."""
    L = geo.pyramid()[-1]
    t0 = trace_of(geo, edits, pts[:1], hint)[0, :3]
    x, y, _p = P.scan_in_map(L, t0, pts)
    return _to_scan(L, t0, np.stack([np.floor(x) + 0.5, np.floor(y) + 0.5], 1)), t0


def inside_scan(geo, n, hint, border=6.0):
    """The first n points of a synthetic scan that the hint's pose puts at least `border` cells inside the finest
    level (the scans reach beyond a 256^2 map)."""
    L = geo.pyramid()[0]
    pts = K.scan(geo.res, min(n + n // 2 + 40, 2000))
    x, y, _p = P.scan_in_map(L, P.map_from_world(L, hint), pts)
    pts = pts[(np.minimum(x, y) > border) & (x < L.sx - 2 - border) & (y < L.sy - 2 - border)][:n]
    assert pts.shape[0] == n, (n, pts.shape)
    return pts


def placed(geo, edits, n, movers, hint, cells=None, same=False, border=6.0):
    """A one-level scan of n points in cell centres (of the first step) that stay in their cells on the second step,
    except the points `movers`: the second step's pose finds each of those in its own cell of the first step -- or in
    `cells` ((x, y) per mover) if given -- but just across the border from where the first step's pose saw it: on the
    axis the pose moves along most, half that move inside the cell (the other axis: the centre).  same: all movers are
    one point.  The pose's move between the two steps follows from the points, so the placement is iterated with the
    oracle.  Returns (pts, trace)."""
    assert geo.levels == 1
    L = geo.pyramid()[0]
    base, t0 = centred(geo, edits, inside_scan(geo, n, hint, border), hint)
    movers = np.asarray(movers, np.int64)
    pts = base.copy()
    if cells is None:
        x, y, _p = P.scan_in_map(L, t0, base[movers])
        cells = np.stack([np.floor(x), np.floor(y)], 1)
    cells = np.asarray(cells, np.float64).reshape(-1, 2)
    for _ in range(40 if movers.size else 0):
        t1 = trace_of(geo, edits, pts, hint)[1, :3]
        x0, y0, _p = P.scan_in_map(L, t0, pts[movers])
        x1, y1, _p = P.scan_in_map(L, t1, pts[movers])
        d = np.stack([x1 - x0, y1 - y0], 1)            # each mover's way between the two steps
        a = int(np.argmax(np.abs(d.mean(0))))
        tgt = cells + 0.5
        tgt[:, a] = cells[:, a] + np.where(d[:, a] > 0, 0.0, 1.0) + 0.5 * d[:, a]
        if same:
            tgt = np.repeat(tgt[:1], movers.size, 0)
        new = _to_scan(L, t1, tgt)
        done = np.abs(new - pts[movers]).max() < 1.0e-4
        pts[movers] = new if done else 0.5 * (new + pts[movers])   # (damped: many movers move the pose themselves)
        if done:
            break
    return pts, trace_of(geo, edits, pts, hint)


# the pose the plain scan matches at: with the points moved to cell centres the first step moves it by about 0.2 cells
# and the later ones hardly at all, so a point in a cell's centre stays in its cell and a placed point changes it
NEAR = K.HINT_TRUE


def _step1(geo, pts, tr):
    miss, packed, mg = misses_of(geo, tr, pts)
    assert packed[1] and mg[:2].min() > MARGIN, mg[:2].min()
    assert np.isfinite(tr[:, :3]).all()
    return miss, packed, mg


class Pair:
    """One single-stream fleet and one oracle on the same maps."""

    def __init__(self, geo, edits):
        self.fleet = HectorFleet(1, geo.res, geo.sx, geo.start, geo.levels, max_points=1152, map_size_y=geo.sy)
        self.ora = geo.oracle()
        K.load(self.ora, geo, edits)
        K.load(self.fleet, geo, edits, stream=0)

    def check(self, pts, hint, origo=(0.0, 0.0), what=""):
        hint = np.asarray(hint, np.float32)
        gp, gc = self.fleet.match(0, pts, hint, origo)
        op, oc = self.ora.match(pts, hint, origo)
        _same_bits(gp, op, f"{what} pose")
        _same_bits(gc, oc, f"{what} covariance")
        assert self.fleet.clamp_count(0) == self.ora.clamp_count(), f"{what} clamp count"
        return gp

    def close(self):
        self.fleet.close()
        self.ora.close()


@pytest.fixture(scope="module")
def pairs(gpu):
    made = {}

    def get(geo, edits=False):
        if (geo, edits) not in made:
            made[(geo, edits)] = Pair(geo, edits)
        return made[(geo, edits)]

    yield get
    for p in made.values():
        p.close()


def test_no_miss_after_the_first_step(pairs):
    """1. Every point in its cell's centre, the pose moves by a fraction of a cell: no list entry, no pass, on any
    of the five packed steps.  Two hints: the pose moves by 0.2 and by 0.45 cells."""
    for n in (300, 1000):
        for hint in (K.HINT_TRUE, (K.HINT_TRUE[0] + 0.012, K.HINT_TRUE[1] + 0.012, K.HINT_TRUE[2])):
            pts, tr = placed(G1, False, n, [], hint)
            miss, packed, mg = misses_of(G1, tr, pts)
            assert not miss[packed].any() and mg.min() > MARGIN and miss[0].sum() > 0.8 * n
            assert np.abs(tr[1:, :3] - tr[0, :3]).max() > 0.0, "the pose moves"
            pairs(G1).check(pts, hint, what=f"no miss, n = {n}")


@pytest.mark.parametrize("lane", [0, 63])
@pytest.mark.parametrize("wave,slot_j", [(0, 0), (2, 1)])
def test_one_miss_in_a_wave(pairs, lane, wave, slot_j):
    """2. Exactly one list entry in one point wave on the second step, from lane 0 or lane 63 (of the first slot of
    wave 0, of the second slot of wave 2); no other wave has one."""
    i = slot_j * CW_PTS + wave * 64 + lane
    pts, tr = placed(G1, False, 400, [i], NEAR)
    miss, _packed, _mg = _step1(G1, pts, tr)
    assert np.flatnonzero(miss[1]).tolist() == [i] and wave_of(i) == wave and lane_of(i) == lane
    pairs(G1).check(pts, NEAR, what=f"one miss, point {i}")


def test_every_lane_of_every_slot_misses(pairs):
    """3. A hint 9 cells off: the first step moves every point by more than a cell, so on the second step every
    lane of all six slots of every wave misses -- six full passes per wave."""
    hint = (K.HINT_TRUE[0] - 0.5, K.HINT_TRUE[1] + 0.8, K.HINT_TRUE[2])
    L = G1.pyramid()[0]
    pts = inside_scan(G1, 1152, hint, border=12.0)
    tr = trace_of(G1, False, pts, hint)
    x0, y0, _p = P.scan_in_map(L, tr[0, :3], pts)
    x1, y1, _p = P.scan_in_map(L, tr[1, :3], pts)
    inside = (np.minimum(x1, y1) > 1.0) & (x1 < L.sx - 3) & (y1 < L.sy - 3)
    assert inside.all() and (np.maximum(np.abs(x1 - x0), np.abs(y1 - y0)) > 1.0 + MARGIN).all()
    pairs(G1).check(pts, hint, what="all miss")


@pytest.mark.parametrize("count", [63, 64, 65, 129])
def test_partial_last_pass(pairs, count):
    """4. 63, 64, 65 and 129 misses in wave 1 on the second step (its other points and the other waves' stay): a
    partial pass, one full pass, a full and a one-entry pass, two full and one."""
    n = 3 * CW_PTS
    own = np.flatnonzero(wave_of(np.arange(n)) == 1)
    movers = np.concatenate([own[own >= CW_PTS][: count - 20], own[:20]])   # slots 1 and 2 first, then 20 lanes of slot 0
    assert movers.size == count
    pts, tr = placed(G1, False, n, movers, NEAR)
    miss, _packed, _mg = _step1(G1, pts, tr)
    assert sorted(np.flatnonzero(miss[1]).tolist()) == sorted(movers.tolist())
    pairs(G1).check(pts, NEAR, what=f"{count} misses in one wave")


# hints tried per point count until the oracle's trajectory has a miss on a packed step
COUNT_HINTS = ((0.33, 0.03, 0.08), (0.36, 0.05, 0.12), (0.25, -0.05, 0.05), (0.4, 0.1, 0.0), (0.2, 0.0, 0.2),
               (0.3, 0.2, 0.3), (0.05, 0.3, -0.1), (0.6, -0.3, 0.1))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 191, 192, 193, 1151, 1152])
def test_point_counts(pairs, n):
    """5. Around a wave (64), a chunk (192) and the register slots (1152), two levels, under a hint with misses on
    the packed steps."""
    geo = K.G256
    pts = K.scan(geo.res, n)
    found = 0
    for hint in COUNT_HINTS:
        miss, packed, _mg = misses_of(geo, trace_of(geo, False, pts, hint), pts)
        if miss[packed].any():
            found += 1
            pairs(geo).check(pts, hint, what=f"n = {n} hint {hint}")
            if found == 2:
                break
    assert found, f"n = {n}: no hint with a miss on a packed step"


@pytest.mark.parametrize("n", [300, 1000])
def test_points_cross_the_map_limits(pairs, n):
    """6. Points inside the map on a level's first step, outside on a later one (no gather: the key turns NB_NONE,
    the cached cell stays) and inside again later (a gather, unless the cell is the cached one)."""
    for case in K.hint_cases():
        if case.expect != "leave_return" or case.n != n or case.geo.levels > 2:
            continue
        K.check_precondition(case)
        tr = trace_of(case.geo, False, case.pts, case.hint)
        cx, _cy, _mg = cells_of(case.geo, tr, case.pts)
        miss, packed, _ = misses_of(case.geo, tr, case.pts)
        lvl0 = slice(cx.shape[0] - 6, cx.shape[0])
        gone = (cx[lvl0][:-1] >= 0) & (cx[lvl0][1:] < 0)
        back = (cx[lvl0][:-1] < 0) & (cx[lvl0][1:] >= 0)
        assert gone.any() and back.any() and (miss[lvl0][1:] & back).any(), case.name
        pairs(case.geo).check(case.pts, case.hint, case.origo, what=case.name)


# cells whose 2 x 2 neighbourhood straddles: the tile seam in x and y, in x only, in y only; 4-cell block seams; the
# map's last neighbourhoods in x and in y; all among the hand-built cells of the 96 x 80 map
SEAM_CELLS = [(63, 31), (63, 30), (62, 31), (64, 31), (3, 3), (7, 7), (7, 8), (3, 4), (93, 5), (10, 77), (64, 32),
              (62, 30), (0, 0)]


def test_missed_cells_on_seams(pairs):
    """7. On the 96 x 80 map with hand-built cells: points that the second step finds in cells whose neighbourhoods
    straddle the 64 x 32 tile seams and 4 x 4 block seams (and end on the map's last column and row), having been
    elsewhere on the first step -- gathered by the packed pass."""
    geo = G96_1
    edits = K.maps(geo, True)[0][0]
    plain = K.maps(geo, False)[0][0]
    for (x, y), in_x, in_y in (((63, 31), True, True), ((63, 30), True, False), ((62, 31), False, True), ((3, 3), True, True)):
        nb = edits[y:y + 2, x:x + 2]   # hand-built values that differ across the seam
        assert (nb != plain[y:y + 2, x:x + 2]).any(), (x, y, nb)
        assert (not in_x or (nb[:, 0] != nb[:, 1]).any()) and (not in_y or (nb[0] != nb[1]).any()), (x, y, nb)
    hint = (0.1, 0.05, -0.05)
    movers = np.arange(len(SEAM_CELLS)) * 3   # lanes 0, 3, .. of wave 0's first slot
    pts, tr = placed(geo, True, 200, movers, hint, cells=SEAM_CELLS, border=2.0)
    miss, packed, mg = misses_of(geo, tr, pts)
    cx, cy, _ = cells_of(geo, tr, pts)
    assert mg[:2, movers].min() > MARGIN and miss[1, movers].all()
    assert [(int(a), int(b)) for a, b in zip(cx[1, movers], cy[1, movers])] == SEAM_CELLS
    pairs(geo, True).check(pts, hint, (1.5, -0.75), what="seams")


def test_one_cell_missed_by_many_lanes(pairs):
    """8. 100 coincident points spread over two waves and three slots change their cell together: 100 list entries
    with one key.  (A hundred points on one spot steer the pose themselves; the spot is the first of the scan's cells
    at which the placement settles.)"""
    movers = np.concatenate([np.arange(10, 50), np.arange(CW_PTS + 70, CW_PTS + 100), np.arange(2 * CW_PTS + 5, 2 * CW_PTS + 35)])
    L = G1.pyramid()[0]
    x, y, _p = P.scan_in_map(L, P.map_from_world(L, NEAR), inside_scan(G1, 600, NEAR))
    for k in range(0, 600, 13):
        pts, tr = placed(G1, False, 600, movers, NEAR, cells=[(np.floor(x[k]), np.floor(y[k]))] * movers.size, same=True)
        miss, packed, mg = misses_of(G1, tr, pts)
        if mg[:2].min() > MARGIN and np.flatnonzero(miss[1]).tolist() == movers.tolist():
            break
    else:
        raise AssertionError("no cell at which 100 coincident points settle")
    assert (pts[movers] == pts[movers[0]]).all() and np.isfinite(tr[:, :3]).all()
    pairs(G1).check(pts, NEAR, what="coincident")


def test_three_levels(pairs):
    """9. The same points through three levels: each level's first step (LDS-DMA) is followed by packed steps with
    misses, and one point keeps its cell -- and so its key -- from one level to the next (the existing case)."""
    for case in K.same_cell_cases():
        if case.geo.levels != 3:
            continue
        K.check_precondition(case)
        miss, packed, _mg = misses_of(case.geo, trace_of(case.geo, True, case.pts, case.hint), case.pts)
        per_level = [miss[a:b][packed[a:b]].sum() for a, b in ((0, 4), (4, 8), (8, 14))]
        assert min(per_level) > 0, per_level
        pairs(case.geo, True).check(case.pts, case.hint, case.origo, what=case.name)
    geo = K.G256.with_levels(3)
    for n, hint in ((1081, (0.33, 0.03, 0.08)), (700, (0.3, 0.2, 0.3))):
        pts = K.scan(geo.res, n)
        miss, packed, _mg = misses_of(geo, trace_of(geo, False, pts, hint), pts)
        assert min(miss[a:b][packed[a:b]].sum() for a, b in ((0, 4), (4, 8), (8, 14))) > 0
        pairs(geo).check(pts, hint, what=f"three levels n = {n}")


def test_batched_ragged_streams(gpu):
    """10. One launch over 40 streams on equal 128^2 maps, each with its own count and hint: every chain wave.  As
    in tests/test_hector_match_gpu.py the first step draws its scan into the map on both sides; then the thresholds
    keep the update away and the second step is a pure match."""
    import torch

    B, geo = 40, K.G128
    assert {(b + (b >> 8)) & 3 for b in range(B)} == {0, 1, 2, 3}
    rng = np.random.default_rng(7)
    counts = rng.choice(np.asarray(K.COUNTS_1152), (2, B)).astype(np.int32)
    counts[1, :12] = (1, 63, 64, 65, 191, 192, 193, 385, 577, 1151, 1152, 960)
    pts = np.zeros((2, B, 1152, 2), np.float32)
    hints = np.zeros((2, B, 3), np.float32)
    for t in range(2):
        for s in range(B):
            pts[t, s, : counts[t, s]] = K.scan(geo.res, int(counts[t, s]), k=4 + t)
        hints[t] = rng.uniform(-1.0, 1.0, (B, 3)) * np.array([0.15, 0.15, 0.1])
    fleet = HectorFleet(B, geo.res, geo.sx, geo.start, geo.levels, max_points=1152, map_size_y=geo.sy)
    fleet.set_update_factors(0.4, 0.9)
    oras = []
    for s in range(B):
        K.load(fleet, geo, stream=s)
        o = geo.oracle()
        o.set_update_factors(0.4, 0.9)
        K.load(o, geo)
        oras.append(o)
    missed = 0
    for t in range(2):
        if t == 1:
            fleet.set_thresholds(1.0e9, 1.0e9)
            for o in oras:
                o.set_thresholds(1.0e9, 1.0e9)
        d_xy, d_n, d_h = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (pts[t], counts[t], hints[t]))
        fleet.step_device(d_xy.data_ptr(), 1152, d_n.data_ptr(), 0, d_h.data_ptr())
        torch.cuda.synchronize()
        gp, gc, gd, _ = fleet.poses()
        for s in range(B):
            p = pts[t, s, : counts[t, s]]
            if t == 1:
                oras[s].enable_trace(64)
            op, oc, od = oras[s].process(p, hint=hints[t, s])
            if t == 1 and np.isfinite(oras[s].trace()[:, :3]).all():
                miss, packed, _mg = misses_of(geo, oras[s].trace(), p)
                missed += bool(miss[packed].any())
            assert bool(gd[s]) == od, (t, s)
            _same_bits(gp[s], op, f"step {t} stream {s} (n = {counts[t, s]}) pose")
            _same_bits(gc[s], oc, f"step {t} stream {s} (n = {counts[t, s]}) covariance")
            assert fleet.clamp_count(s) == oras[s].clamp_count(), (t, s)
    assert missed >= B // 2, missed
    fleet.close()
    for o in oras:
        o.close()
