"""Directed inputs for the Hector grid update (hs_update_kernel, hs_update_ring_kernel, hs_bin_kernel + hs_tile_kernel),
chosen from the kernels' own structure, and reach(): the CPU-side facts that show a case gets where it claims.

A Case is a map geometry, an optional table of log-odds loaded before the first update, and a list of updates (scan,
pose, origo).  Points are in level-0 cells.  The builder places the begin cell by choosing the pose -- map coordinates
(bx + 0.25, by + 0.25), a quarter cell off the centre so that no level's coordinate sits on a cell border -- and
asserts the resulting begin and end cells with the plain statement (tests/ref/hector_update_plain.py); nothing here
derives them by a formula of its own.

A Path is a way through the host's launch logic: environment variables read at hs_create and the max_points that
selects the kernel instance.  admits() and shmem_bytes() restate the host's limits (hector_internal.h plan_step);
parts() restates upd_split and the SLAM2D_UPD_PARTS parse (parse_options).  tests/test_hector_launch_cpu.py holds all
of them, and the constants below, to the library's own header on the CPU.

replay(case) runs the oracle and the plain statement side by side, update by update, records every difference and
returns the facts per update and level (cached: the CPU tests share one replay per case).
"""
import dataclasses
import functools

import numpy as np

import oracle as O
import hector_update_plain as P

F = np.float32
RES = 0.05
FREE, OCC = 0.4, 0.9
TILE, TILE_H = 64, 32
NAN, INF = float("nan"), float("inf")
# csrc/hector_internal.h: UPD_THREADS, UPD_STRIDE, UPD_TH, UPD_HIT_WORDS, UPD_MARK_WORDS, UPD_FIXED_WORDS, UPD_GROUP_WORDS
UPD_THREADS = 256
UPD_MARK_WORDS = (32 * 68 + 32 * 2 + 3) & ~3
UPD_FIXED_WORDS = 2 * UPD_MARK_WORDS + 4
REG_POINTS = 1280   # UPD_RREG * 256: the register instance's (and the ring kernel's) largest scan
MAX_BIN_TILES = 1024


@dataclasses.dataclass(frozen=True)
class Geo:
    name: str
    sx: int
    sy: int
    levels: int
    start: tuple = (0.5, 0.5)


G1 = Geo("G1", 40, 30, 1, (0.3, 0.6))
G2A = Geo("G2a", 70, 18, 1, (0.5, 0.5))
G2B = Geo("G2b", 18, 70, 1, (0.7, 0.2))
G3 = Geo("G3", 65, 33, 1, (0.5, 0.5))
G4 = Geo("G4", 96, 80, 3, (0.4, 0.55))
G5X = Geo("G5x", 16385, 64, 2, (0.01, 0.5))
G5Y = Geo("G5y", 64, 16385, 2, (0.5, 0.99))
G5RX = Geo("G5rx", 16384, 64, 2, (0.01, 0.5))
G5RY = Geo("G5ry", 64, 16384, 2, (0.5, 0.99))
G6X = Geo("G6x", 4096, 160, 1, (0.02, 0.5))
G6Y = Geo("G6y", 160, 4096, 1, (0.5, 0.02))
G7 = Geo("G7", 2112, 1056, 1, (0.5, 0.5))


@dataclasses.dataclass
class Update:
    pts: np.ndarray
    pose: np.ndarray
    origo: tuple = (0.0, 0.0)
    begin: tuple = None          # the level-0 begin cell the builder asserted (None: not directed)
    ends: list = None            # the level-0 end cells it asserted (None entries: not asserted)


@dataclasses.dataclass
class Case:
    name: str
    kind: str
    geo: Geo
    updates: list
    init: str = None             # None | "values" | "sparse"
    env: dict = dataclasses.field(default_factory=dict)   # beyond the path's (SLAM2D_ORD_SWEEP)

    @property
    def n_max(self):
        return max(len(u.pts) for u in self.updates)


def plain_map(geo):
    return P.PlainMap(RES, geo.sx, geo.sy, geo.start, geo.levels, FREE, OCC)


def place(geo, bx, by, theta=0.0):
    """The world pose whose level-0 map coordinates are (bx + 0.25, by + 0.25, theta)."""
    L = plain_map(Geo("", geo.sx, geo.sy, 1, geo.start)).lv[0]
    return np.asarray([(bx + 0.25 - float(L.tx)) / float(L.scale), (by + 0.25 - float(L.ty)) / float(L.scale), theta], F)


def directed(geo, begin, ends, origo=(0.0, 0.0), pose_begin=None):
    """One update from the begin cell to the given level-0 targets.  A target is a cell (ints) or a pair of map
    coordinates (floats, the value before the + 0.5); the end cells the plain statement gets are asserted for the cell
    targets and recorded for the others."""
    bx, by = pose_begin if pose_begin is not None else begin
    pose = place(geo, bx, by)
    pts = np.zeros((len(ends), 2), F)
    want = []
    for i, (ex, ey) in enumerate(ends):
        cell = isinstance(ex, (int, np.integer)) and isinstance(ey, (int, np.integer))
        pts[i] = (ex - bx, ey - by) if cell else (ex - (bx + 0.25), ey - (by + 0.25))
        want.append((int(ex), int(ey)) if cell else None)
    got_begin, got = plain_map(Geo("", geo.sx, geo.sy, 1, geo.start)).end_cells(0, pts, pose, origo)
    assert got_begin == tuple(begin), (got_begin, begin)
    for w, g in zip(want, got):
        assert w is None or w == g, (w, g)
    return Update(pts, pose, origo, tuple(begin), got)


# ---------------------------------------------------------------------------------------------- scans
ORDERS = ("row_major", "reversed", "permuted", "far_first", "near_first")


def ordered(cells, begin, order):
    cheb = lambda c: max(abs(c[0] - begin[0]), abs(c[1] - begin[1]))  # noqa: E731
    if order == "row_major":
        return list(cells)
    if order == "reversed":
        return list(cells)[::-1]
    if order == "permuted":
        rng = np.random.default_rng(977 + begin[0] * 131 + begin[1])
        return [cells[i] for i in rng.permutation(len(cells))]
    if order == "far_first":      # every end cell (but the outermost) was freed by an earlier, longer beam
        return sorted(cells, key=lambda c: -cheb(c))
    if order == "near_first":     # every end cell is hit before a later beam would free it
        return sorted(cells, key=cheb)
    raise ValueError(order)


def every_cell(geo, begin, orders=ORDERS, split=None, tag=""):
    """One beam to every cell of the level-0 map but the begin cell, once per order (consecutive updates of one map);
    split: scans of at most that many beams (the register instance and the ring kernel hold 1280)."""
    cells = [(x, y) for y in range(geo.sy) for x in range(geo.sx) if (x, y) != tuple(begin)]
    ups = []
    for o in orders:
        seq = ordered(cells, begin, o)
        k = 1 if not split else -(-len(seq) // split)
        per = -(-len(seq) // k)
        for j in range(k):
            ups.append(directed(geo, begin, seq[j * per:(j + 1) * per]))
    return Case(f"every_{geo.name}_{begin[0]}_{begin[1]}{tag}", "every_cell", geo, ups)


def begins(geo):
    """A corner, the opposite corner, both sides of the tile seams (where the map has them), the centre."""
    out = [(0, 0), (geo.sx - 1, geo.sy - 1)]
    sx_seam, sy_seam = geo.sx > TILE, geo.sy > TILE_H
    if sx_seam or sy_seam:
        out.append((63 if sx_seam else geo.sx // 2, 31 if sy_seam else geo.sy // 2))
        other = (64 if sx_seam else geo.sx // 2 - 1, 32 if sy_seam else geo.sy // 2 - 1)
        out.append(other if other not in out else (other[0], other[1] - 1))   # (G3's far corner is (64, 32))
    out.append((geo.sx // 2, geo.sy // 2))
    return out


STAR_H = (1, 2, 3, 31, 32, 33, 63, 64, 65)


def perimeter(c, h):
    x0, y0 = c
    out = [(x0 + h, y0 + t) for t in range(-h, h)] + [(x0 - t, y0 + h) for t in range(-h, h)]
    out += [(x0 - h, y0 - t) for t in range(-h, h)] + [(x0 + t, y0 - h) for t in range(-h, h)]
    return out


def star(geo, begin):
    """The perimeters of the squares of half-width STAR_H around the begin cell, clipped to the map; then the same
    points from the same place turned by 0.4 rad (cells by cos and sin, not by construction)."""
    ends = [c for h in STAR_H for c in perimeter(begin, h) if 0 <= c[0] < geo.sx and 0 <= c[1] < geo.sy]
    u0 = directed(geo, begin, ends)
    u1 = Update(u0.pts, place(geo, begin[0], begin[1], 0.4))
    return Case(f"star_{geo.name}", "star", geo, [u0, u1])


def edge_targets(geo, begin):
    sx, sy = geo.sx, geo.sy
    # some in-map coordinate other than the begin cell's
    mx, my = (begin[0] + 1, begin[1] + 1) if begin[0] + 1 < sx and begin[1] + 1 < sy else (sx // 2, sy // 2)
    mid = lambda v: v + 0.25  # noqa: E731  (map coordinate in the middle of cell v's range after + 0.5)
    t = []
    # exactly on the four borders (and the four corners)
    t += [(0, my), (sx - 1, my), (mx, 0), (mx, sy - 1), (0, 0), (sx - 1, 0), (0, sy - 1), (sx - 1, sy - 1)]
    # one cell beyond each: cancelled
    t += [(mid(-2), mid(my)), (mid(sx), mid(my)), (mid(mx), mid(-2)), (mid(mx), mid(sy))]
    # map coordinates in (-1.5, -0.5]: -1 < v + 0.5 <= 0, which (int) truncates toward zero into cell 0 -- drawn
    for v in (-0.7, -1.4, -0.5, -1.49):
        t += [(v, mid(my)), (mid(mx), v), (v, v)]
    t += [(-1.5, mid(my))]   # -1.0 up to rounding: whichever cell the float sum gives
    # nothing a cell can hold
    for v in (NAN, INF, -INF, 1e10, -1e10):
        t += [(v, mid(my)), (mid(mx), v), (v, v)]
    # begin == end, by the centre and by another point of the same cell
    t += [(mid(begin[0]), mid(begin[1])), (begin[0] + 0.4, begin[1] - 0.1)]
    return t


def edges(geo):
    """Border, beyond-border, truncated, non-finite and begin == end end points from an inner begin cell; the same
    points with the begin cell outside the map, through the origo and through the pose; the begin cell on the last
    row and column."""
    b = (geo.sx // 2 - 3, geo.sy // 2 + 2)
    u0 = directed(geo, b, edge_targets(geo, b))
    far = (float(geo.sx + 9), 0.0)
    u1 = directed(geo, (b[0] + geo.sx + 9, b[1]), edge_targets(geo, b), origo=far, pose_begin=b)     # out by the origo
    # out by the pose: map coordinate -2.75, and (int)(-2.25) is cell -2
    u2 = directed(geo, (-2, geo.sy // 2), [(5, 5), (0, 0), (geo.sx - 1, geo.sy - 1)], pose_begin=(-3, geo.sy // 2))
    last = (geo.sx - 1, geo.sy - 1)
    u3 = directed(geo, last, edge_targets(geo, last))
    return Case(f"edges_{geo.name}", "edges", geo, [u0, u1, u2, u3])


LIMIT_DB = (0, 1, 2, 3, 31, 32, 33, 62, 63)
G6_DB_MID = (0, 1, 2, 3, 31, 32, 33, 62, 63, 64, 65, 78, 79)
G6_DB_SIDE = (0, 1, 63, 64, 65, 127, 128, 129, 157, 158, 159)


def limit_update(geo, sa, b0, dbs_signed):
    """From the begin cell at one end of the long axis (a) to the far end: da in {limit, limit - 1, limit - 2, 8191,
    8192, 8193} (the limit is the long side - 1) with every signed db of the list, then 64 neighbouring rays (one
    fan: forward and backward lanes) three cells short of the middle."""
    x_long = geo.sx > geo.sy
    la, lb = (geo.sx, geo.sy) if x_long else (geo.sy, geo.sx)
    lim = la - 1
    half = 8192 if lim > 8193 else lim // 2
    das = (lim, lim - 1, lim - 2, half - 1, half, half + 1)
    a0 = 0 if sa > 0 else lim
    ab = lambda a, b: (a, b) if x_long else (b, a)  # noqa: E731
    ends = [ab(a0 + sa * da, b0 + db) for db in dbs_signed for da in das]
    nb = [b for b in range(max(0, b0 - 63), min(lb, b0 + 64))][:64]
    ends += [ab(a0 + sa * (half - 3), b) for b in nb]
    assert all(0 <= e[0] < geo.sx and 0 <= e[1] < geo.sy for e in ends)
    return directed(geo, ab(a0, b0), ends), sum(das) * len(dbs_signed)


def limit(geo):
    lb = min(geo.sx, geo.sy)
    ups = []
    if lb == 64:   # G5 / G5r: the four sign combinations from the four corners
        plan = [(1, 0, LIMIT_DB), (1, 63, [-d for d in LIMIT_DB]), (-1, 0, LIMIT_DB), (-1, 63, [-d for d in LIMIT_DB])]
    else:          # G6: the middle of a short side (both db signs in one scan), then its corners (db up to 159)
        both = [s * d for d in G6_DB_MID for s in (1, -1) if d or s > 0]
        plan = [(1, lb // 2, both), (-1, lb // 2, both), (1, 0, G6_DB_SIDE), (-1, lb - 1, [-d for d in G6_DB_SIDE])]
    da_sum = []
    for sa, b0, dbs in plan:
        u, s = limit_update(geo, sa, b0, dbs)
        ups.append(u)
        da_sum.append(s)
    c = Case(f"limit_{geo.name}", "limit", geo, ups)
    c.da_sum = da_sum
    return c


def many_distinct(n):
    """500 distinct end cells of G1's map visited cyclically: consecutive beams always differ, so nu = n."""
    begin = (G1.sx // 2, G1.sy // 2)
    cells = [(x, y) for y in range(G1.sy) for x in range(G1.sx)]
    cells.sort(key=lambda c: (-max(abs(c[0] - begin[0]), abs(c[1] - begin[1])), c))
    ring = sorted(cells[:500], key=lambda c: np.arctan2(c[1] - begin[1], c[0] - begin[0]))
    return Case(f"many_{n}", "many_distinct", G1, [directed(G1, begin, [ring[i % 500] for i in range(n)])])


def _f32(bits):
    return np.asarray([bits], np.uint32).view(F)[0]


def value_table():
    lf, lo = P.prob_to_logodds(FREE), P.prob_to_logodds(OCC)
    t = [F(0.0), F(-0.0), _f32(1), F(1e-38), F(-1e-38), lf, -lf, F(1e-8), F(49.999996), F(50.0),
         np.nextafter(F(50.0), F(60.0)), F(50.0) - lo, F(1e30), F(-1e30), F(INF), F(-INF), _f32(0x7FC12345),
         _f32(0x7FA00001)]
    assert (F(1e-8) + lf) - lf != F(1e-8) and t[8] < F(50.0) < t[10]
    return np.asarray(t, F)


VALUE_STRIDE = (5, 7)   # the table entry of cell (x, y) is (5 x + 7 y) mod 18


def init_levels(case):
    """[(log-odds, updateIndex)] per level to load before the first update (never-updated index planes)."""
    if case.init is None:
        return None
    out = []
    for lvl in range(case.geo.levels):
        sx, sy = case.geo.sx >> lvl, case.geo.sy >> lvl
        y, x = np.mgrid[0:sy, 0:sx]
        if case.init == "values":
            t = value_table()
            l = t[(VALUE_STRIDE[0] * x + VALUE_STRIDE[1] * y) % len(t)]
        else:   # sparse: every cell a quiet NaN whose payload is the cell's own number
            l = (np.uint32(0x7FC00000) | (1 + y * sx + x).astype(np.uint32)).view(F)
        out.append((np.ascontiguousarray(l, F), np.full((sy, sx), -1, np.int32)))
    return out


def values(geo, order):
    """Perimeters 3 cells apart around the centre on a map loaded with value_table(): far-first the inner perimeters'
    cells were freed by the outer beams (freed-then-hit), the outermost are hit only and the cells between are free
    only; near-first every end cell is hit only."""
    begin = (geo.sx // 2, geo.sy // 2)
    hs = range(2, max(geo.sx, geo.sy), 3)
    ends = [c for h in hs for c in perimeter(begin, h) if 0 <= c[0] < geo.sx and 0 <= c[1] < geo.sy]
    ends = ordered(ends, begin, order)
    return Case(f"values_{geo.name}_{order}", "values", geo, [directed(geo, begin, ends)], init="values")


def sparse(geo, sweep):
    """Three steep rays down one column of quads (x in [4 k, 4 k + 3]): one, two or three cells of each quad drawn, the
    rest payload NaNs; then a second update up the same column drawing other cells of the same quads."""
    k4 = 60 if geo.sx > TILE else 16
    top, bot = 0, geo.sy - 1
    u0 = directed(geo, (k4 + 1, top), [(k4 + 1, bot), (k4 + 2, bot), (k4 + 3, bot)])
    u1 = directed(geo, (k4, bot), [(k4, top), (k4 + 2, top)])
    return Case(f"sparse_{geo.name}_sweep{sweep}", "sparse", geo, [u0, u1], init="sparse",
                env={"SLAM2D_ORD_SWEEP": str(sweep)})


G7B = Geo("G7b", 2048, 1024, 1, (0.5, 0.5))   # 32 x 32 tiles: exactly MAX_BIN_TILES, still binned by tile


def g7_corners(geo=G7):
    b = (geo.sx // 2, geo.sy // 2)
    ends = [(0, 0), (geo.sx - 1, 0), (0, geo.sy - 1), (geo.sx - 1, geo.sy - 1)]
    return Case(f"{geo.name.lower()}_corners", "g7", geo, [directed(geo, b, ends)])


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = []
    for geo in (G1, G2A, G2B, G3):
        for b in begins(geo):
            cs.append(every_cell(geo, b))
    for b in begins(G3):   # G3's 2144 beams in scans the register instance and the ring kernel hold
        cs.append(every_cell(G3, b, split=REG_POINTS, tag="_split"))
    for i, b in enumerate(begins(G4)):   # two orders per begin cell, all five over the six cases
        cs.append(every_cell(G4, b, orders=(ORDERS[(2 * i) % 5], ORDERS[(2 * i + 1) % 5])))
    for geo in (G1, G2A, G2B, G3, G4):
        cs.append(edges(geo))
    cs.append(star(G1, (G1.sx // 2, G1.sy // 2)))
    cs.append(star(G2A, (64, 9)))
    cs.append(star(G2B, (9, 31)))
    cs.append(star(G3, (63, 32)))
    cs.append(star(G4, (64, 31)))
    cs.append(star(G6X, (2048, 80)))
    for geo in (G5X, G5Y, G5RX, G5RY, G6X, G6Y):
        cs.append(limit(geo))
    for geo in (G1, G4):
        for o in ("far_first", "near_first"):
            cs.append(values(geo, o))
        for sweep in (1, 2):
            cs.append(sparse(geo, sweep))
    for n in (4096, 4097, 4160, 10000):
        cs.append(many_distinct(n))
    cs.append(g7_corners())
    cs.append(g7_corners(G7B))
    assert len({c.name for c in cs}) == len(cs)
    return {c.name: c for c in cs}


# ---------------------------------------------------------------------------------------------- paths
@dataclasses.dataclass(frozen=True)
class Path:
    name: str
    env: tuple = ()
    inst: str = "auto"    # "regs": max_points <= 1280; "lds": max_points >= 1281; "auto": the scan's own size
    kernel: str = "clip"  # "clip" | "ring" | "binned"

    def max_points(self, case):
        n = max(case.n_max, 16)
        return max(n, REG_POINTS + 1) if self.inst == "lds" else n

    def shmem_bytes(self, case):
        """plan_step's shmem: the mark buffers, the rays (LDS instance) and a box per fan group."""
        mp = self.max_points(case)
        rays = 0 if mp <= REG_POINTS else (mp + 3) & ~3
        return 4 * (UPD_FIXED_WORDS + rays + 4 * (-(-mp // UPD_THREADS) * 4))

    def admits(self, case):
        g, mp = case.geo, self.max_points(case)
        if self.kernel == "binned":
            return True
        if max(g.sx, g.sy) > 16385 or self.shmem_bytes(case) > 65536 or case.kind == "g7":
            return False
        if self.inst == "regs" and mp > REG_POINTS:
            return False
        if self.kernel == "ring":   # larger scans fall back to hs_update_kernel<0> under the ring setting: not ring coverage
            return mp <= REG_POINTS and max(g.sx, g.sy) <= 16384
        return True

    def fixed_parts(self, levels):
        env = dict(self.env)
        if "SLAM2D_UPD_PARTS" not in env:
            return None
        v = [min(64, max(1, int(t))) for t in env["SLAM2D_UPD_PARTS"].split(",")]
        return [v[min(l, len(v) - 1)] for l in range(levels)]

    def parts(self, levels, ncu, U=1):
        """Workgroups per (stream, level): SLAM2D_UPD_PARTS, else upd_split for U updating streams."""
        fp = self.fixed_parts(levels)
        if fp is not None:
            return fp
        env = dict(self.env)
        minp = [int(t) for t in env.get("SLAM2D_UPD_SPLIT", "0").split(",")]
        minp = [min(64, max(0, minp[l])) if l < len(minp) else 0 for l in range(levels)]
        p0 = max(2, ((2 if U <= 32 else 4) * ncu + U - 1) // U)
        if levels == 1:
            p0 = max(p0, 8)
        return [min(64, max(1, max(p0 >> l, minp[l]))) for l in range(levels)]


PATHS = {p.name: p for p in (
    Path("regs", inst="regs"),
    Path("lds", inst="lds"),
    Path("parts1", (("SLAM2D_UPD_PARTS", "1"),)),
    Path("parts321", (("SLAM2D_UPD_PARTS", "3,2,1"),)),
    Path("parts64", (("SLAM2D_UPD_PARTS", "64"),)),
    Path("split532", (("SLAM2D_UPD_SPLIT", "5,3,2"),)),
    Path("ring", (("SLAM2D_UPD_KERNEL", "ring"),), kernel="ring"),
    Path("ring_p1", (("SLAM2D_UPD_KERNEL", "ring"), ("SLAM2D_UPD_PARTS", "1")), kernel="ring"),
    Path("ring_p4", (("SLAM2D_UPD_KERNEL", "ring"), ("SLAM2D_UPD_PARTS", "4")), kernel="ring"),
    Path("ring_p64", (("SLAM2D_UPD_KERNEL", "ring"), ("SLAM2D_UPD_PARTS", "64")), kernel="ring"),
    Path("binned", (("SLAM2D_UPDATE", "binned"),), kernel="binned"),
)}
MAIN_PATHS = ("regs", "lds", "parts1", "ring", "binned")


def plan():
    """[(path, case)] the GPU file runs.  every_cell on G1 to G3, edges and values: every path that admits them (all
    begin cells on the main paths, the seam and centre cells on the others); limit: its own kernel's rows; many_distinct:
    the clip rows that admit it; star: the main paths."""
    out = []
    for cn, c in all_cases().items():
        for pn, p in PATHS.items():
            if not p.admits(c):
                continue
            main = pn in MAIN_PATHS
            if c.kind == "every_cell":
                if c.geo is G4 and pn not in ("lds", "parts1", "parts321", "binned"):
                    continue
                if c.geo is G3 and pn in ("lds", "binned") and cn.endswith("_split"):
                    continue   # (the unsplit case runs there)
                if not main and c.updates[0].begin not in begins(c.geo)[2:]:
                    continue
            elif c.kind == "star" and not main:
                continue
            elif c.kind == "limit":
                ring_geo = c.geo in (G5RX, G5RY)
                ok = {"parts1", "parts64", "split532", "lds", "regs"} if not ring_geo else {"ring", "ring_p1", "ring_p4", "ring_p64", "regs"}
                if c.geo in (G6X, G6Y):
                    ok = {"regs", "parts1", "ring", "ring_p4", "binned"}
                if pn not in ok:
                    continue
            elif c.kind == "many_distinct" and pn not in ("lds", "parts1", "split532"):
                continue
            elif c.kind == "g7" and pn != "binned":
                continue
            out.append((pn, cn))
    return out


# ---------------------------------------------------------------------------------------------- reach
def survivors(rays):
    """tests/test_ray_dedup_cpu.py::survivors: a beam is kept when it is drawn and its ray differs from its predecessor's."""
    return [r for b, r in enumerate(rays) if r is not None and (b == 0 or r != rays[b - 1])]


def level_facts(rec, sx, detail=False):
    begin, ends = rec["begin"], rec["ends"]
    ff, fh = rec["first_free"], rec["first_hit"]
    valid = [e for e in ends if e is not None]
    f = dict(begin=begin, n=rec["n"], valid=len(valid), nu=len(survivors(ends)), ntx=0, nty=0, ntiles=0, da_max=0, kmax=0)
    if valid:
        xs = [begin[0]] + [e[0] for e in valid]
        ys = [begin[1]] + [e[1] for e in valid]
        f["ntx"] = max(xs) // TILE - min(xs) // TILE + 1
        f["nty"] = max(ys) // TILE_H - min(ys) // TILE_H + 1
        f["ntiles"] = f["ntx"] * f["nty"]
        f["da_max"] = max(max(abs(e[0] - begin[0]), abs(e[1] - begin[1])) for e in valid)
        btx, bty = begin[0] // TILE, begin[1] // TILE_H
        f["kmax"] = max(max(abs(x // TILE - btx) for x in xs), max(abs(y // TILE_H - bty) for y in ys))  # rings - 1
    marked = set(ff) | set(fh)
    quads = {}
    for off in marked:
        quads.setdefault(off // sx * sx + (off % sx) // 4 * 4, []).append(off)
    f["quad_full"] = sum(len(v) == 4 for v in quads.values())
    f["quad_part"] = sum(len(v) < 4 for v in quads.values())
    f["quad_hit"] = sum(any(o in fh for o in v) for v in quads.values())
    f["quad_nohit"] = len(quads) - f["quad_hit"]
    f["hit_freed_earlier"] = sum(o in ff and ff[o] < fh[o] for o in fh)
    f["hit_freed_later"] = sum(o in ff and ff[o] > fh[o] for o in fh)
    if detail:   # per cell (values and sparse cases: small maps)
        f["outcome"] = {o: ("free" if o not in fh else ("freed_hit" if o in ff and ff[o] < fh[o] else "hit")) for o in marked}
        f["quads"] = quads
    return f


def tiles_per_workgroup(f, parts):
    """The most tiles one workgroup of the clip kernel owns: tiles t = part, part + parts, ... of the box."""
    return -(-f["ntiles"] // parts) if f["ntiles"] else 0


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def make_oracle(geo):
    o = O.HectorOracle(RES, geo.sx, geo.start, geo.levels, reduce_threads=0, map_size_y=geo.sy)
    o.set_update_factors(FREE, OCC)
    o.set_thresholds(-1.0, -1.0)
    return o


def touched_since(ora, levels, base):
    """Cells the oracle's last update changed: their updateIndex is one of its two marks (base[lvl] + 1, + 2)."""
    return sum(int((ora.level(lvl)[1] > base[lvl]).sum()) for lvl in range(levels))


@functools.lru_cache(maxsize=None)
def replay(name):
    """Oracle and plain statement through the case, update by update.  Returns (differences, facts): facts[k][lvl]
    = level_facts of update k, plus facts[k]["counters"]."""
    case = all_cases()[name]
    geo = case.geo
    ora, pl = make_oracle(geo), plain_map(geo)
    diffs, facts = [], []
    init = init_levels(case)
    for k, u in enumerate(case.updates):
        if geo.levels > 1:   # matchData stores the container the coarse levels draw (its pose is not the subject)
            ora.match(u.pts, u.pose, u.origo)
            pl.store_container(u.pts, u.origo)
        if k == 0 and init:
            for lvl, (l, ui) in enumerate(init):
                ora.set_level(lvl, l, ui)
                pl.set_level(lvl, l, ui)
        base = [ora.cur_update_index(lvl) for lvl in range(geo.levels)]
        ora.update_by_scan(u.pts, u.pose, u.origo)
        pl.update_by_scan(u.pts, u.pose, u.origo)
        fk = {}
        for lvl in range(geo.levels):
            ol, ou = ora.level(lvl)
            ql, qu = pl.level(lvl)
            if not np.array_equal(_bits(ol), _bits(ql)):
                diffs.append(f"update {k} level {lvl}: log-odds")
            if not np.array_equal(ou, qu):
                diffs.append(f"update {k} level {lvl}: updateIndex")
            if ora.update_index(lvl) != pl.lv[lvl].last or ora.cur_update_index(lvl) != pl.lv[lvl].cur:
                diffs.append(f"update {k} level {lvl}: update_index")
            if not np.array_equal(ora.publish(lvl), pl.publish(lvl)):
                diffs.append(f"update {k} level {lvl}: publish bytes")
            fk[lvl] = level_facts(pl.lv[lvl].rec, pl.lv[lvl].sx, detail=case.init is not None)
            pl.lv[lvl].rec = None
        got = dict(cells=ora.sum_L(), rays=ora.valid_rays(), touched=touched_since(ora, geo.levels, base))
        want = dict(cells=pl.cells, rays=pl.rays, touched=pl.touched)
        if got != want:
            diffs.append(f"update {k}: counters {got} != {want}")
        fk["counters"] = got
        facts.append(fk)
    return diffs, facts


def reach(case, path=None, ncu=256):
    """The facts of replay(case), with the tiles per workgroup under the path's parts added per level."""
    _, facts = replay(case.name)
    if path is not None and path.kernel == "clip":
        parts = path.parts(case.geo.levels, ncu)
        for fk in facts:
            for lvl in range(case.geo.levels):
                fk[lvl]["tiles_per_wg"] = tiles_per_workgroup(fk[lvl], parts[lvl])
    return facts


# ---------------------------------------------------------------------------------------------- batch
def batch_scans():
    """Six ragged streams on G4's map, each another case's scan (two of them empty), and per step the hints: the
    streams whose hint moves by a metre pass the update gate at thresholds (0.4, 0.9), the others do not.  The
    non-finite targets are left out of the edges scan: the matcher's pose of such a scan is NaN, and the batch compares
    poses."""
    b = (G4.sx // 2, G4.sy // 2)
    e = edges(G4).updates[0]
    keep = np.isfinite(e.pts).all(axis=1) & (np.abs(e.pts) < 1e6).all(axis=1)
    ups = [every_cell(G4, b, orders=("row_major",)).updates[0], star(G4, (64, 31)).updates[0],
           Update(e.pts[keep], e.pose), None, every_cell(G4, (0, 0), orders=("far_first",)).updates[0], None]
    scans = [u.pts if u else np.zeros((0, 2), F) for u in ups]
    scans[4] = scans[4][:3000]   # (the longest 3000 beams of the far-first order)
    poses = [u.pose if u else place(G4, 10, 10) for u in ups]
    moved = [(False, False), (True, False), (False, True), (True, True), (True, True), (False, False)]
    hints = np.zeros((3, 6, 3), F)
    for t in range(3):
        for s in range(6):
            hints[t, s] = poses[s]
            if t and moved[s][t - 1]:
                hints[t, s, 0] += F(1.0 * t)   # a metre (20 cells) per step
    return scans, hints
