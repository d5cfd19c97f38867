"""Inputs of tests/test_gmapping_paths_gpu.py and of the builder checks in tests/test_gmapping_cpu.py: plain numpy.

Directed beams.  gm_set_beams takes arbitrary (a_cos, a_sin); they need not be unit vectors.  With the pose
(px, py, 1, 0) at the centre of cell p0 = (x0, y0) and a_cos[b] = (x1 - x0) delta / d, a_sin[b] = (y1 - y0) delta / d,
beam b ends at the centre of cell (x1, y1): a hit when its range is d < max_urange, a miss (clamped, d = max_urange)
for any range in (max_urange, max_range].  A pose (px, py, -1, 0) mirrors every offset about p0.  Every case therefore
knows its end cells as integers, and check_intent() proves from the oracle alone that the oracle's hit cells are those.

A case holds one beam cache and up to three steps of P <= 4 poses; oracle_maps() computes the oracle's maps once per
case and keeps them unchanged for every test that needs them.
"""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass, field

import numpy as np

import oracle as O

TILE_W, TILE_H = 64, 32   # gm_compute_kernel's tile (gmapping_internal.h)

_RANGES = dict(max_range=30 - 0.01, max_urange=25.0)
GEOMS = {
    # the reference's launch geometry: 1600 x 1600 cells centred on the origin
    "default": dict(O.GM_DEFAULTS),
    # 96 x 64 cells off-centre: 2 x 2 tiles, the last tile column 32 cells wide; most 500-cell lines leave the map
    "small_offset": dict(_RANGES, xmin=10.0, xmax=14.8, ymin=-7.0, ymax=-3.8, delta=0.05),
    # 4096 x 1024 cells: max_range / delta ~ 6000, in-map lines of 3000-4000 cells
    "fine_long": dict(_RANGES, xmin=-10.24, xmax=10.24, ymin=-2.56, ymax=2.56, delta=0.005),
}


def dims(p):
    """(sx, sy, sx2, sy2, cx, cy) of a parameter dict."""
    sx, sy, sx2, sy2 = O.gm_geometry(p)
    return sx, sy, sx2, sy2, (p["xmin"] + p["xmax"]) / 2.0, (p["ymin"] + p["ymax"]) / 2.0


def cell_pose(p, x0, y0, flip=False):
    """The pose at the centre of cell (x0, y0), heading +x (or -x: every beam offset mirrored)."""
    _, _, sx2, sy2, cx, cy = dims(p)
    return [cx + (x0 - sx2) * p["delta"], cy + (y0 - sy2) * p["delta"], -1.0 if flip else 1.0, 0.0]


def cround(x):
    """C round(): half away from zero (numpy's rounds half to even)."""
    x = np.asarray(x, np.float64)
    t = np.trunc(x)
    return (t + np.sign(x) * (np.abs(x - t) >= 0.5)).astype(np.int64)


def end_cells(p, pose4, ranges, a_cos, a_sin):
    """ComputeMap's per-beam filter and end cell (gmapping.cc:183-214) in numpy doubles: (valid, hit, x, y)."""
    _, _, sx2, sy2, cx, cy = dims(p)
    px, py, ct, st = (float(v) for v in pose4)
    d = np.asarray(ranges, np.float32).astype(np.float64)
    n = len(d)
    ca, sa = np.asarray(a_cos, np.float64)[:n], np.asarray(a_sin, np.float64)[:n]
    with np.errstate(invalid="ignore"):
        valid = ~((d > p["max_range"]) | (d == 0.0) | ~np.isfinite(d))
        d = np.where(valid, np.where(d > p["max_urange"], p["max_urange"], d), 0.0)
    hit = valid & (d < p["max_urange"])
    wx = px + d * (ct * ca - st * sa)
    wy = py + d * (st * ca + ct * sa)
    return valid, hit, cround((wx - cx) / p["delta"]) + sx2, cround((wy - cy) / p["delta"]) + sy2


def expected_score(prev, pose4, ranges, a_cos, a_sin, p=O.GM_DEFAULTS, thresh=0.25):
    """Hit beams whose end cell is occupied (n / visits > thresh) in the previous map (n, visits), or 0 without one."""
    if prev is None:
        return 0
    n_prev, v_prev = prev
    sx, sy = dims(p)[:2]
    _, hit, x, y = end_cells(p, pose4, ranges, a_cos, a_sin)
    ok = hit & (x >= 0) & (x < sx) & (y >= 0) & (y < sy)
    x, y = x[ok], y[ok]
    v = v_prev[y, x].astype(np.float64)
    occ = np.where(v > 0, n_prev[y, x].astype(np.float64) * 1 / np.where(v > 0, v, 1.0), -1.0)
    return int((occ > thresh).sum())


def publish(n, v, thresh=0.25):
    """gmo_publish of a dense map."""
    out = np.empty(n.shape, np.int8)
    O.gmapping_oracle_lib().gmo_publish(O._fp(np.ascontiguousarray(n)), O._fp(np.ascontiguousarray(v)), n.shape[1],
                                        n.shape[0], thresh, O._fp(out))
    return out


@dataclass
class Step:
    poses4: np.ndarray    # [P, 4]
    p0: np.ndarray        # [P, 2] the poses' cells
    flip: np.ndarray      # [P] offsets mirrored
    ranges: np.ndarray    # float32 [n], n <= len(a_cos)
    hit: np.ndarray       # bool [n]: the beams meant to be hits


@dataclass
class Case:
    name: str
    gname: str
    p: dict
    a_cos: np.ndarray
    a_sin: np.ndarray
    offsets: np.ndarray   # int [nb, 2] end cell - p0 of every beam
    steps: list = field(default_factory=list)

    def hit_ends(self, s, k):
        """The intended end cells [h, 2] of step s, particle k's hit beams, in beam order (in the map or not)."""
        st = self.steps[s]
        off = self.offsets[: len(st.ranges)][st.hit]
        return st.p0[k] + (-off if st.flip[k] else off)

    def intended_n(self, s, k):
        """The hit counts the case means to produce: a histogram of hit_ends inside the map."""
        sx, sy = dims(self.p)[:2]
        e = self.hit_ends(s, k)
        e = e[(e[:, 0] >= 0) & (e[:, 0] < sx) & (e[:, 1] >= 0) & (e[:, 1] < sy)]
        n = np.zeros((sy, sx), np.int32)
        np.add.at(n, (e[:, 1], e[:, 0]), 1)
        return n


def plain_ranges(p, hit, hit_range=8.0):
    """(ranges float32, effective d) of directed beams: hits at hit_range (scalar or per beam), misses at a range
    between max_urange and max_range, which ComputeMap clamps to max_urange."""
    hit = np.asarray(hit, bool)
    miss = np.float32(0.5 * (p["max_urange"] + p["max_range"]))
    r = np.where(hit, np.broadcast_to(np.asarray(hit_range, np.float32), hit.shape), miss).astype(np.float32)
    return r, np.where(hit, r.astype(np.float64), p["max_urange"])


def build(name, gname, offsets, ranges, d_eff, hit, steps, frac=None):
    """steps: [(poses [(x0, y0, flip), ...], n or None, drop or None)]; a dropped beam gets range 0.  d_eff is the
    distance each beam travels (its range, or max_urange when clamped); frac [nb, 2] moves end points inside their
    cells (|frac| < 0.5)."""
    p = GEOMS[gname]
    offsets = np.asarray(offsets, np.int64).reshape(-1, 2)
    ranges = np.asarray(ranges, np.float32)
    hit = np.asarray(hit, bool)
    off = offsets.astype(np.float64) + (0.0 if frac is None else np.asarray(frac, np.float64))
    d = np.asarray(d_eff, np.float64)
    c = Case(name, gname, p, off[:, 0] * p["delta"] / d, off[:, 1] * p["delta"] / d, offsets)
    for poses, n, drop in steps:
        n = len(ranges) if n is None else n
        r, h = ranges[:n].copy(), hit[:n].copy()
        if drop is not None:
            r[drop[:n]] = 0.0
            h[drop[:n]] = False
        c.steps.append(Step(np.asarray([cell_pose(p, x, y, f) for x, y, f in poses], np.float64),
                            np.asarray([(x, y) for x, y, _ in poses], np.int64),
                            np.asarray([f for _, _, f in poses], bool), r, h))
    return c


# ------------------------------------------------------------------------------------------------ families
def _octant_offsets():
    out = []
    for a, b in [(7, 0), (7, 7), (7, 3), (70, 69), (130, 1), (1, 0), (0, 0)]:
        for sa, sb in itertools.product((1, -1), (1, -1)):
            for o in ((sa * a, sb * b), (sb * b, sa * a)):
                if o not in out:
                    out.append(o)
    return out


def octants(gname):
    """The eight octants, the dy == dx tie, a1 == a0 (axis-aligned), a one-cell and a zero-length beam: every end
    once as a hit and once as a miss, from a p0 on a tile's last row and column and from one on its first."""
    p = GEOMS[gname]
    offs = [o for o in _octant_offsets() for _ in (0, 1)]
    hit = np.arange(len(offs)) % 2 == 0
    r, d = plain_ranges(p, hit, np.resize(np.asarray([1.0, 8.0, 24.5], np.float32), len(offs)))
    corner = (831, 831) if gname == "default" else (63, 31)   # x % 64 == 63, y % 32 == 31
    poses = [(corner[0], corner[1], False), (corner[0] + 1, corner[1] + 1, False)]
    return build(f"octants_{gname}", gname, offs, r, d, hit, [(poses, None, None)])


LONG_P0 = (100, 900)


def long_line_offsets(rng, n_random=200):
    sx, sy = dims(GEOMS["fine_long"])[:2]
    x0, y0 = LONG_P0
    ends = np.stack([rng.integers(-200, sx + 200, n_random), rng.integers(-200, sy + 200, n_random)], axis=1)
    directed = [(x0 + 3999, y0 + 1), (x0 + 3999, y0 - 1), (x0 + 3999, y0 - 3998), (x0 + 3998, y0 - 3999),
                (x0 + 3999, y0), (x0, y0 - 900), (0, 0), (sx - 1, 0), (0, sy - 1), (sx - 1, sy - 1),
                (x0 + 3000, y0 - 900), (x0 + 3999, y0 - 3999), (x0 + 1, y0 - 900), (x0 + 3995, y0 - 2)]
    return np.concatenate([ends, np.asarray(directed)]) - np.asarray(LONG_P0)


def long_lines():
    """Lines of up to 4000 cells in the map (6000 leaving it) on fine_long, from near one corner and, mirrored, from
    near the opposite one; a second step from the middle of the map."""
    p = GEOMS["fine_long"]
    sx, sy = dims(p)[:2]
    rng = np.random.default_rng(2024)
    offs = long_line_offsets(rng)
    hit = rng.random(len(offs)) < 0.5
    hit[200:] = np.arange(len(offs) - 200) % 2 == 0
    r, d = plain_ranges(p, hit, rng.choice(np.asarray([0.5, 8.0, 24.5], np.float32), len(offs)))
    x0, y0 = LONG_P0
    steps = [([(x0, y0, False), (sx - 1 - x0, sy - 1 - y0, True)], None, None),
             ([(sx // 2, sy // 2, True), (x0, y0, True)], None, None)]
    return build("long_lines", "fine_long", offs, r, d, hit, steps)


STEEP_DA = (4280, 4416, 4540, 4556, 4802, 5000, 5241, 5600, 5988, 5990)


def steep_entering():
    """Lines of slope 2 (dy = -2 dx, 4280 to 5990 cells) whose far end lies up to 5000 cells below the map: the walk
    starts at that end, so the steps inside the map are steps 3000 to 5990 of the line and the clip's numerators
    2 da t (t: a tile column's offset from the start) reach 3.5e7 in tiles that the line crosses.  With 2 db == da
    every tile-column boundary gives a numerator of the form k d - 1 above 2^24, which rounds up to k d as a float:
    the float quotient estimate is then k, one too high, for any reciprocal that is not rounded down (and for many
    of these divisors even then).  A clip that is one step off either skips a free cell or counts one too many."""
    p = GEOMS["fine_long"]
    offs = [(sg * (da // 2), -da) for da in STEEP_DA for sg in (1, -1)]
    hit = np.arange(len(offs)) % 4 < 2
    r, d = plain_ranges(p, hit, 24.5)
    return build("steep_entering", "fine_long", offs, r, d, hit, [([(100, 1010, False), (3990, 1010, False)], None, None)])


def _filler(rng, nb, span, avoid):
    """nb random offsets within +-span cells, none of them in `avoid`."""
    offs = rng.integers(-span, span + 1, (nb, 2))
    for i in range(nb):
        while tuple(offs[i]) in avoid:
            offs[i] = rng.integers(-span, span + 1, 2)
    return offs


MULTI_P0 = (40, 20)
MULTI_C1, MULTI_C1_BEAMS, MULTI_C1_MISS = (70, 40), (10, 11, 80, 310, 910), 200
MULTI_C2, MULTI_C2_BEAMS = (10, 5), (12, 333, 640, 1005)


def multi_hit():
    """A 1081-beam scan on small_offset: cell C1 hit by beams b, b+1, b+70, b+300, b+900 (different fan groups and
    waves) at five points inside it, a miss ending in C1 between them; cell C2, in the first tile, hit by four beams
    spread over the scan.  Every other beam is a random hit or miss elsewhere."""
    p = GEOMS["small_offset"]
    rng = np.random.default_rng(31)
    nb = 1081
    o1 = (MULTI_C1[0] - MULTI_P0[0], MULTI_C1[1] - MULTI_P0[1])
    o2 = (MULTI_C2[0] - MULTI_P0[0], MULTI_C2[1] - MULTI_P0[1])
    offs = _filler(rng, nb, 60, {o1, o2})
    hit = rng.random(nb) < 0.6
    for b in MULTI_C1_BEAMS + (MULTI_C1_MISS,):
        offs[b] = o1
        hit[b] = b != MULTI_C1_MISS
    for b in MULTI_C2_BEAMS:
        offs[b] = o2
        hit[b] = True
    frac = rng.uniform(-0.45, 0.45, (nb, 2))
    r, d = plain_ranges(p, hit, rng.choice(np.asarray([1.0, 8.0, 24.5], np.float32), nb))
    poses = [(MULTI_P0[0], MULTI_P0[1], False), (MULTI_P0[0] + 1, MULTI_P0[1] + 1, False)]
    return build("multi_hit", "small_offset", offs, r, d, hit, [(poses, None, None)], frac=frac)


def hit_points(case, s, k, beams):
    """The float32 hit points (as PointAccumulator receives them) of the given beams of step s, particle k."""
    st = case.steps[s]
    px, py, ct, _ = st.poses4[k]
    d = st.ranges[list(beams)].astype(np.float64)
    return np.stack([(px + d * (ct * case.a_cos[list(beams)])).astype(np.float32),
                     (py + d * (ct * case.a_sin[list(beams)])).astype(np.float32)], axis=1)


def order_sensitive(points):
    """True when some order of the float32 points sums (sequentially, from 0) to another value than the given one."""
    def fsum(seq):
        a = np.zeros(2, np.float32)
        for q in seq:
            a = (a + q).astype(np.float32)
        return a.view(np.int32).tolist()
    ref = fsum(points)
    return any(fsum([points[i] for i in perm]) != ref for perm in itertools.permutations(range(len(points))))


TSEQ_BOX = (4, 3)       # tiles
TSEQ_OFF = (17, 9)      # in-tile offset of every hit cell
TSEQ_T0 = (10, 20)      # first tile of the box (default geometry)


def tile_sequence(rising):
    """parts = 1 walks the tiles of the box in order.  One hit cell per tile of a 4 x 3 tile box, all at the same
    in-tile offset, i.e. the same first-hit and count words of LDS in consecutive tiles; the hitting beam's index
    rises (or falls) with the tile index, 70 beams apart, so it changes fan group and wave.  All other beams are
    dropped (range 0).  p0 is the first tile's cell."""
    p = GEOMS["default"]
    ntx, nty = TSEQ_BOX
    nt = ntx * nty
    nb = 70 * nt
    x0, y0 = TSEQ_T0[0] * TILE_W + TSEQ_OFF[0], TSEQ_T0[1] * TILE_H + TSEQ_OFF[1]
    offs = np.zeros((nb, 2), np.int64)
    drop = np.ones(nb, bool)
    for t in range(nt):
        b = 70 * (t if rising else nt - 1 - t) + 3
        offs[b] = ((t % ntx) * TILE_W, (t // ntx) * TILE_H)
        drop[b] = False
    hit = ~drop
    r, d = plain_ranges(p, hit)
    poses = [(x0, y0, False), (x0 + 3 * TILE_W, y0 + 2 * TILE_H, True)]
    return build(f"tile_seq_{'rising' if rising else 'falling'}", "default", offs, r, d, hit, [(poses, None, drop)])


def tile_alternating():
    """Two beams from the middle of a 3 x 3 tile box to its opposite corners, one a hit and one a miss: in box order
    the tiles alternate marked / unmarked, with a hit tile and free-only tiles.  A second step swaps hit and miss
    (new beams), so the first step's hit tile is free-only and the flags of both parities have carried both values."""
    p = GEOMS["default"]
    x0, y0 = 11 * TILE_W + 32, 21 * TILE_H + 16
    offs = [(TILE_W + 20, TILE_H + 10), (-(TILE_W + 20), -(TILE_H + 10)), (TILE_W + 20, TILE_H + 10),
            (-(TILE_W + 20), -(TILE_H + 10))]
    hit = np.asarray([True, False, False, True])
    r, d = plain_ranges(p, hit)
    poses = [(x0, y0, False), (x0 + 7, y0 + 3, True)]
    d1 = np.asarray([False, False, True, True])
    return build("tile_alternating", "default", offs, r, d, hit, [(poses, None, d1), (poses, None, ~d1)])


def one_tile():
    """Every line inside one tile: with parts = 16, fifteen of the sixteen workgroups have no tile."""
    p = GEOMS["small_offset"]
    rng = np.random.default_rng(8)
    offs = rng.integers(-9, 10, (90, 2))
    hit = rng.random(90) < 0.5
    r, d = plain_ranges(p, hit)
    return build("one_tile", "small_offset", offs, r, d, hit, [([(20, 12, False)], None, None)])


EDGE_NAMES = ("0", "-0", "nan", "+inf", "-inf", "max_range", "above_max_range", "max_urange", "below_max_urange", "-3")


def range_edges():
    """One beam per special range value, between ordinary beams.  Valid in the reference: everything but d > maxRange,
    d == 0 and non-finite; so a negative range is a hit, max_range (as float32, just below the double) a clamped miss,
    max_urange exactly a miss and the float below it a hit."""
    p = GEOMS["small_offset"]
    rng = np.random.default_rng(77)
    mr, mu = np.float32(p["max_range"]), np.float32(p["max_urange"])
    special = np.asarray([0.0, -0.0, np.nan, np.inf, -np.inf, mr, np.nextafter(mr, np.float32(np.inf)), mu,
                          np.nextafter(mu, np.float32(0)), -3.0], np.float32)
    assert float(mr) <= p["max_range"] < float(special[6]) and float(mu) == p["max_urange"]
    s_hit = np.asarray([0, 0, 0, 0, 0, 0, 0, 0, 1, 1], bool)
    s_d = np.asarray([1, 1, 1, 1, 1, p["max_urange"], 1, p["max_urange"], float(special[8]), -3.0], np.float64)
    nb = 3 * len(special)
    offs = _filler(rng, nb, 30, set())
    hit = rng.random(nb) < 0.5
    r, d = plain_ranges(p, hit)
    at = np.arange(len(special)) * 3 + 1
    r[at], d[at], hit[at] = special, s_d, s_hit
    return build("range_edges", "small_offset", offs, r, d, hit, [([(30, 40, False), (70, 20, True)], None, None)])


def own_cell():
    """All 1081 beams end in p0's own cell (0.01 m ranges): no free cell; one cell with n = visits = 1081 and the
    float sum of 1081 hit points in beam order."""
    p = GEOMS["small_offset"]
    rng = np.random.default_rng(5)
    nb = 1081
    hit = np.ones(nb, bool)
    r, d = plain_ranges(p, hit, 0.01)
    return build("own_cell", "small_offset", np.zeros((nb, 2), np.int64), r, d, hit, [([(50, 33, False)], None, None)],
                 frac=rng.uniform(-0.45, 0.45, (nb, 2)))


def scan_n(n):
    """n beams of a 1081-beam cache: the beams past n must not exist (they are hits all over the map)."""
    p = GEOMS["small_offset"]
    rng = np.random.default_rng(100 + n)
    nb = 1081
    offs = _filler(rng, nb, 40, set())
    hit = rng.random(nb) < 0.6
    r, d = plain_ranges(p, hit)
    return build(f"scan_n{n}", "small_offset", offs, r, d, hit, [([(33, 31, False), (64, 32, True)], n, None)])


def stale_tiles():
    """Score and stale tiles (default geometry): A and B have disjoint tile boxes.  Steps A, B, A, A, then at A two
    beams to opposite corners of A's box; the second particle goes B, A, B, B likewise."""
    p = GEOMS["default"]
    rng = np.random.default_rng(12)
    nb = 300
    offs = _filler(rng, nb, 100, set())
    offs[nb - 2], offs[nb - 1] = (100, 100), (-100, -100)
    hit = rng.random(nb) < 0.7
    hit[nb - 2:] = (True, False)
    r, d = plain_ranges(p, hit)
    a, b = (300, 300, False), (1300, 1300, False)
    last = np.ones(nb, bool)
    last[nb - 2:] = False
    return build("stale_tiles", "default", offs, r, d, hit,
                 [([a, b], None, None), ([b, a], None, None), ([a, b], None, None), ([a, b], None, None),
                  ([a, b], None, last)])


THRESH_P0, THRESH_X, THRESH_Y = (10, 10), (20, 10), (10, 20)


def threshold():
    """Step 1 (both particles at p0) leaves cell X at n = 1, visits = 4 and cell Y at n = 2, visits = 4: one / two
    hits on the cell and three / two misses running through it.  Step 2 is the one hit beam on X (beam 0): particle 0
    stays, particle 1 stands where the same beam ends in Y."""
    p = GEOMS["small_offset"]
    offs = [(10, 0), (20, 0), (21, 0), (22, 0), (0, 10), (0, 10), (0, 20), (0, 21)]
    hit = np.asarray([1, 0, 0, 0, 1, 1, 0, 0], bool)
    r, d = plain_ranges(p, hit)
    p0 = (THRESH_P0[0], THRESH_P0[1], False)
    p1 = (THRESH_Y[0] - 10, THRESH_Y[1], False)
    return build("threshold", "small_offset", offs, r, d, hit, [([p0, p0], None, None), ([p0, p1], 1, None)])


def partial():
    """Five particles on small_offset, three different scans (drop masks) of one 200-beam cache."""
    p = GEOMS["small_offset"]
    rng = np.random.default_rng(9)
    nb = 200
    offs = _filler(rng, nb, 45, set())
    hit = rng.random(nb) < 0.7
    r, d = plain_ranges(p, hit)
    poses = [(20 + 13 * k, 12 + 9 * k, k % 2 == 1) for k in range(5)]
    moved = [(x + 3, y - 2, f) for x, y, f in poses]
    return build("partial", "small_offset", offs, r, d, hit,
                 [(poses, None, rng.random(nb) < 0.2), (moved, 150, rng.random(nb) < 0.2), (poses, None, None)])


def in_map_beams(gname, k):
    """Directed and random beams that keep every line inside the map (the reference asserts on cells outside it):
    the inputs of the committed reference fixture and of the live reference comparison.  k = 0, 1: two poses."""
    p = GEOMS[gname]
    sx, sy = dims(p)[:2]
    rng = np.random.default_rng(500 + k)
    if gname == "fine_long":
        x0, y0, flip = (LONG_P0[0], LONG_P0[1], False) if k == 0 else (sx - 1 - LONG_P0[0], sy - 1 - LONG_P0[1], True)
        ends = [LONG_P0, (4095, 901), (4095, 899), (4095, 0), (0, 0), (0, 1023), (101, 0), (100, 0), (900, 100)]
        ends += [(int(rng.integers(0, sx)), int(rng.integers(0, sy))) for _ in range(2)]
        offs = np.asarray(ends) - np.asarray(LONG_P0)
    else:
        x0, y0, flip = (63, 31, False) if k == 0 else (64, 32, True)
        sgn = -1 if flip else 1
        offs = np.asarray([o for o in _octant_offsets() + [tuple(v) for v in rng.integers(-95, 96, (60, 2))]
                           if 0 <= x0 + sgn * o[0] < sx and 0 <= y0 + sgn * o[1] < sy])
    hit = np.arange(len(offs)) % 3 != 2
    r, d = plain_ranges(p, hit, np.resize(np.asarray([1.0, 8.0, 24.5], np.float32), len(offs)))
    c = build(f"in_map_{gname}_{k}", gname, offs, r, d, hit, [([(x0, y0, flip)], None, None)])
    e = c.steps[0].p0[0] + (-c.offsets if flip else c.offsets)
    assert (e >= 0).all() and (e[:, 0] < sx).all() and (e[:, 1] < sy).all()
    return c


BUILDERS = {
    "octants_default": lambda: octants("default"),
    "octants_small_offset": lambda: octants("small_offset"),
    "long_lines": long_lines,
    "steep_entering": steep_entering,
    "multi_hit": multi_hit,
    "tile_seq_rising": lambda: tile_sequence(True),
    "tile_seq_falling": lambda: tile_sequence(False),
    "tile_alternating": tile_alternating,
    "one_tile": one_tile,
    "range_edges": range_edges,
    "own_cell": own_cell,
    **{f"scan_n{n}": functools.partial(scan_n, n) for n in (1, 63, 64, 65, 257)},
    "stale_tiles": stale_tiles,
    "threshold": threshold,
    "partial": partial,
}
# the families run at every SLAM2D_GM_PARTS; the last three have tests of their own
FAMILY_CASES = [k for k in BUILDERS if k not in ("stale_tiles", "threshold", "partial")]


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def oracle_maps(name):
    """[step][particle] -> (n, visits, acc, nfree, nhits) of the oracle: computed once, shared, never modified."""
    c = case(name)
    out = []
    for st in c.steps:
        n = len(st.ranges)
        row = []
        for pose in st.poses4:
            m = O.gm_compute(st.ranges, c.a_cos[:n], c.a_sin[:n], tuple(pose), p=c.p)
            for a in m[:3]:
                a.setflags(write=False)
            row.append(m)
        out.append(row)
    return out


def check_intent(name):
    """From the oracle alone: its hit cells and counts are the ones the case intends."""
    c = case(name)
    maps = oracle_maps(name)
    for s, st in enumerate(c.steps):
        for k in range(len(st.poses4)):
            np.testing.assert_array_equal(maps[s][k][0], c.intended_n(s, k), err_msg=f"{name} step {s} particle {k}")
            assert maps[s][k][4] == int(st.hit.sum()), (name, s, k)


def tile_kinds(n, v, box=None):
    """Per tile 'h' (some hit), 'f' (visits only) or '.' (no mark), rows of the tile box (default: the marked box)."""
    sy, sx = v.shape
    ty, tx = -(-sy // TILE_H), -(-sx // TILE_W)
    kinds = [["." for _ in range(tx)] for _ in range(ty)]
    for j in range(ty):
        for i in range(tx):
            sl = (slice(j * TILE_H, (j + 1) * TILE_H), slice(i * TILE_W, (i + 1) * TILE_W))
            kinds[j][i] = "h" if n[sl].any() else ("f" if v[sl].any() else ".")
    if box is None:
        ys, xs = np.nonzero(v)
        box = (xs.min() // TILE_W, ys.min() // TILE_H, xs.max() // TILE_W, ys.max() // TILE_H)
    return ["".join(kinds[j][box[0]:box[2] + 1]) for j in range(box[1], box[3] + 1)]
