"""The Karto occupancy-grid rebuild without a GPU: the CPU restatement tests/ref/karto_grid_ref.c against its golden
file and against counts typed out by hand from Grid::TraceLine / OccupancyGrid::RayTrace (Karto.h:4680-4745,
:5910-5945), and the closed form of csrc/karto_grid_line.h (what kg_trace_kernel walks) against the literal loop.
open_karto needs boost and is not built here; the hand-written cases pin the restatement to the reference text, and
the plain float64 model tests/ref/karto_grid_plain.py pins its geometry.  The directed cases of the GPU file (scan-list
rounds, long lines, map and beam edges) are held here to the paths they are named for.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import karto_grid_plain as P  # noqa: E402
import karto_grid_ref as R  # noqa: E402


def test_restatement_reproduces_golden():
    cases = R.load_golden()
    assert set(cases) == set(R.golden_cases())
    for name, (c, want) in cases.items():
        fresh = R.golden_cases()[name]
        np.testing.assert_array_equal(np.asarray(c["ranges"]).view(np.int64), fresh["ranges"].view(np.int64), err_msg=name)
        np.testing.assert_array_equal(c["poses"], fresh["poses"], err_msg=name)
        R.assert_maps_equal(R.create_from_scans(c), want)


def test_golden_holds_numeric_arrays_only():
    z = np.load(R.GOLDEN, allow_pickle=False)
    for k in z.files:
        assert z[k].dtype.kind in "fiuU", (k, z[k].dtype)
    assert os.path.getsize(R.GOLDEN) < 256 * 1024


# ------------------------------------------------------------------ hand-written RayTrace cases (not from the restatement)
def test_hand_horizontal_ray_valid_end():
    ps, ht = R.ray_trace_cells(5, 1, 0, 0, 4, 0, True)
    assert ps.tolist() == [[1, 1, 1, 1, 2]]
    assert ht.tolist() == [[0, 0, 0, 0, 1]]
    ps, ht = R.ray_trace_cells(5, 1, 0, 0, 4, 0, False)
    assert ps.tolist() == [[1, 1, 1, 1, 1]] and ht.sum() == 0


def test_hand_diagonal_ray():
    """|dy| == |dx| is not steep; 2 * error >= deltaX carries at every step."""
    ps, ht = R.ray_trace_cells(4, 4, 0, 0, 3, 3, True)
    assert ps.tolist() == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 2]]
    assert ht.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]]


def test_hand_steep_ray_towards_minus_y():
    """(2, 5) -> (1, 0): steep, then the ends swap, so the walk starts at the END cell (1, 0) with ystep +1:
    error 1, 2, 3 -> the carry comes after the third point; points (1,0) (1,1) (1,2) (2,3) (2,4) (2,5)."""
    assert R.literal_line(2, 5, 1, 0).tolist() == [[1, 0], [1, 1], [1, 2], [2, 3], [2, 4], [2, 5]]
    ps, ht = R.ray_trace_cells(3, 6, 2, 5, 1, 0, True)
    want = np.zeros((6, 3), np.uint32)
    for x, y in [(1, 0), (1, 1), (1, 2), (2, 3), (2, 4), (2, 5)]:
        want[y, x] = 1
    want[0, 1] = 2  # the end point's second pass++
    np.testing.assert_array_equal(ps, want)
    assert ht[0, 1] == 1 and ht.sum() == 1


def test_hand_zero_length_ray():
    ps, ht = R.ray_trace_cells(5, 4, 3, 2, 3, 2, True)
    assert ps[2, 3] == 2 and ps.sum() == 2 and ht[2, 3] == 1 and ht.sum() == 1
    ps, ht = R.ray_trace_cells(5, 4, 3, 2, 3, 2, False)
    assert ps[2, 3] == 1 and ps.sum() == 1 and ht.sum() == 0


def test_hand_cells_off_the_grid_are_skipped():
    """Negative coordinates and an end cell past the width: no increment, no hit (IsValidGridIndex)."""
    ps, ht = R.ray_trace_cells(3, 1, -2, 0, 2, 0, True)
    assert ps.tolist() == [[1, 1, 2]] and ht.tolist() == [[0, 0, 1]]
    ps, ht = R.ray_trace_cells(3, 1, 0, 0, 4, 0, True)
    assert ps.tolist() == [[1, 1, 1]] and ht.sum() == 0


def test_hand_thresholds_case():
    """case_thresholds' cells, counted by hand (see its docstring)."""
    e = R.create_from_scans(R.case_thresholds())
    assert (e["width"], e["height"]) == (70, 70)
    assert (e["pass"][30, 50], e["hits"][30, 50], e["state"][30, 50], e["ros"][30, 50]) == (10, 1, 255, 0)   # 1/10 is not > 0.1
    assert (e["pass"][50, 30], e["hits"][50, 30], e["state"][50, 30], e["ros"][50, 30]) == (9, 1, 100, 100)  # 1/9 is
    assert (e["pass"][30, 20], e["state"][30, 20], e["ros"][30, 20]) == (2, 0, -1)     # pass 2 is not > 2: unknown
    assert (e["pass"][20, 30], e["state"][20, 30], e["ros"][20, 30]) == (3, 255, 0)    # pass 3: free
    assert (e["pass"][30, 0], e["hits"][30, 0], e["state"][30, 0]) == (4, 2, 100)      # the -x end: two scans, two hits
    assert e["pass"][30, 30] == 9 + 8 + 2 + 3                                          # the scans' cell: one per traced ray
    alt = R.create_from_scans(R.case_thresholds(4, 0.5))
    assert alt["state"][20, 30] == 0 and alt["state"][30, 50] == 255 and alt["state"][30, 0] == 0  # 4 is not > 4
    assert alt["state"][50, 30] == 255  # 1/9 is not > 0.5


# ------------------------------------------------------------------ closed form against the literal loop
def _same_line(x0, y0, x1, y1):
    lit = R.literal_line(x0, y0, x1, y1)
    np.testing.assert_array_equal(R.closed_line(x0, y0, x1, y1), lit, err_msg=str((x0, y0, x1, y1)))
    return lit


def _as_sorted_rows(a):
    a = np.asarray(a)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


@pytest.mark.parametrize("origin", [(0, 0), (-37, 91), (70, -129)])
def test_closed_form_every_short_segment(origin):
    """Every segment with both deltas in [-24, 24]: the same points in the same order; and the per-tile walk
    (clip in closed form + incremental loop) over 8 x 8 tiles emits each of them exactly once."""
    x0, y0 = origin
    for dx in range(-24, 25):
        for dy in range(-24, 25):
            lit = _same_line(x0, y0, x0 + dx, y0 + dy)
            tiled = R.tiled_line(x0, y0, x0 + dx, y0 + dy, tile=8)
            np.testing.assert_array_equal(_as_sorted_rows(tiled), _as_sorted_rows(lit), err_msg=str((origin, dx, dy)))


def test_closed_form_random_long_segments():
    """2000 seeded segments with |delta| up to 4000, and 40 beyond the 32-bit path (deltaX > 32767)."""
    rng = np.random.default_rng(20)
    segs = [tuple(int(v) for v in np.concatenate([rng.integers(-3000, 3000, 2), rng.integers(-4000, 4001, 2)]))
            for _ in range(2000)]
    segs += [tuple(int(v) for v in np.concatenate([rng.integers(-3000, 3000, 2), rng.integers(-900000, 900001, 2)]))
             for _ in range(40)]
    for x0, y0, dx, dy in segs:
        lit = _same_line(x0, y0, x0 + dx, y0 + dy)
        tiled = R.tiled_line(x0, y0, x0 + dx, y0 + dy, tile=64 if max(abs(dx), abs(dy)) <= 4000 else 4096)
        np.testing.assert_array_equal(_as_sorted_rows(tiled), _as_sorted_rows(lit), err_msg=str((x0, y0, dx, dy)))


def test_reading_rules_by_hand():
    """case_rules on the restatement: which beams are traced, clipped and score a hit (AddScan, Karto.h:5869-5887)."""
    c = R.case_rules()
    e = R.create_from_scans(c)
    traced = [i for i, r in R.RULES_READINGS.items() if not (r <= R.RULES_MIN or r >= R.RULES_MAX or np.isnan(r))]
    assert sorted(set(range(24)) - set(traced)) == [2, 4, 5, 8, 9, 10]  # NaN, inf, 0, negative, == min, == max
    valid = [i for i in traced if R.RULES_READINGS[i] < R.RULES_THR - 1e-6]
    assert 14 not in valid and 13 not in valid and 16 in valid          # the band [thr - 1e-6, thr) scores no hit
    ends = {i: R.beam_cell(c, e, 0, i, R.RULES_READINGS[i]) for i in valid}
    on_map = [i for i, (x, y) in ends.items() if 0 <= x < e["width"] and 0 <= y < e["height"]]
    assert 16 in on_map and 18 not in on_map                            # the box's own maximum rounds to index == height
    assert int(e["hits"].sum()) == len(on_map)
    x, y = ends[16]
    assert (e["pass"][y, x], e["hits"][y, x]) == (2, 1)                 # just below the band: a hit
    x, y = R.beam_cell(c, e, 0, 14, R.RULES_READINGS[14])
    assert (e["pass"][y, x], e["hits"][y, x]) == (1, 0)                 # in the band: traced unclipped, no hit
    ox, oy = R.beam_cell(c, e, 0, 0, 0.0)
    assert e["pass"][oy, ox] == len(traced)                             # every traced ray starts at the scan's cell


# ------------------------------------------------------------------ the directed cases take the paths they are named for
@functools.lru_cache(maxsize=None)
def _built(kind, *args):
    """case, restatement map and ray cells of a directed case, computed once and shared (treat as read-only)."""
    c = {"rounds": R.case_rounds, "one_pose": lambda S: R.case_rounds(S, one_pose=True), "dims": R.case_dims,
         "beams": R.case_beams}[kind](*args)
    e = R.create_from_scans(c)
    return c, e, R.ray_cells(c, e)


@functools.lru_cache(maxsize=1)
def _built_long(orientation):
    """The same for a long-line case; one at a time (a map is 13 M cells, 130 MB of planes)."""
    c = R.case_long_lines(orientation)
    e = R.create_from_scans(c)
    return c, e, R.ray_cells(c, e)


def _parts(count, split):
    """kg_trace_kernel's share of the scans per part: per = ceil(count / split), part p takes [p * per, ...)."""
    per = (count + split - 1) // split
    return per, [max(0, min(p * per + per, count) - p * per) for p in range(split)]


@pytest.mark.parametrize("S", [257, 513, 600])
def test_rounds_case_takes_later_rounds(S):
    c, e, rc = _built("rounds", S)
    assert len(c["poses"]) == S and -(-S // R.ROUNDS_FIRST) == {257: 2, 513: 3, 600: 3}[S]
    assert np.all(np.isfinite(c["poses"])) and np.nanmax(c["ranges"]) <= R.ROUNDS_REACH
    assert (-(-e["width"] // 64), -(-e["height"] // 64)) == (2, 2) and e["width"] % 64 and e["height"] % 64
    assert np.all(rc[..., 4] >= 0)                        # every beam is traced
    # no scan of the first round reaches the right-hand tile column; scans of every later round do
    assert rc[:R.ROUNDS_FIRST, :, [0, 2]].max() < 64
    for lo in range(R.ROUNDS_FIRST, S, R.ROUNDS_FIRST):
        assert rc[lo:lo + R.ROUNDS_FIRST, :, 0].max() >= 64, lo
    assert e["pass"][:, 64:].sum() > 0 and e["pass"][:, :64].sum() > 0 and e["hits"].sum() > 0
    # and the left-hand column is met in the later rounds too (257: the second round is the one scan at the far end)
    assert S == 257 or rc[R.ROUNDS_FIRST:, :, [0, 2]].min() < 64


def test_rounds_case_partitions():
    """Forced splits over 600, 513 and 257 scans by the kernel's own formula: a part longer than one round, a
    shorter last part, empty parts.  (600 scans over 32 parts leave none empty: 31 * 19 < 600.)"""
    assert _parts(600, 1) == (600, [600])
    per, n = _parts(600, 2)
    assert per == 300 > R.ROUNDS_FIRST and n == [300, 300]
    per, n = _parts(600, 3)
    assert per == 200 and n == [200] * 3
    per, n = _parts(600, 32)
    assert per == 19 and n[:31] == [19] * 31 and n[31] == 11
    per, n = _parts(513, 2)
    assert per == 257 > R.ROUNDS_FIRST and n == [257, 256]
    per, n = _parts(513, 32)
    assert per == 17 and n[30] == 3 and n[31] == 0          # a remainder and an empty part
    per, n = _parts(257, 32)
    assert per == 9 and n[28] == 5 and n[29:] == [0, 0, 0]  # three empty parts
    per, n = _parts(257, 3)
    assert per == 86 and n == [86, 86, 85]


def test_rounds_one_pose_contended_cell():
    c, e, rc = _built("one_pose", 600)
    assert np.all(rc[..., 4] >= 0) and len({tuple(v) for v in rc[..., :2].reshape(-1, 2).tolist()}) == 1
    ox, oy = rc[0, 0, :2]
    assert e["pass"][oy, ox] == 600 * 7 == e["pass"].max()


@pytest.mark.parametrize("orientation", R.LONG_ORIENTATIONS)
def test_long_lines_case_and_tiled_walk(orientation):
    """The case holds what it is named for, and the per-tile walk of csrc/karto_grid_line.h (host build) emits
    the literal loop's cells for every ray the GPU test will walk."""
    c, e, rc = _built_long(orientation)
    assert c["resolution"] == R.LONG_RES and np.all(np.isfinite(c["poses"]))
    assert 0 < e["width"] * e["height"] <= 1 << 24 and e["pass"].sum() > 0 and e["hits"].sum() > 0
    rays = rc.reshape(-1, 5)
    rays = rays[rays[:, 4] >= 0]
    assert len(rays) == 26                                   # 27 readings, one NaN
    dx, dy = rays[:, 2] - rays[:, 0], rays[:, 3] - rays[:, 1]
    major, minor = np.maximum(np.abs(dx), np.abs(dy)), np.minimum(np.abs(dx), np.abs(dy))
    assert {32767, 32768} <= set(major.tolist()) and major.max() >= 40000 and major.min() > 32000
    assert major.max() >= 44990 and minor.max() > 100          # the reading clipped to range_threshold, 45000 cells
    if orientation == "slant":
        assert minor.min() > 0 and minor.max() > 300
    else:
        assert major.max() == 45000 and minor.min() == 0
    steep = np.abs(dy) > np.abs(dx)
    assert np.all(steep) if orientation == "y" else not np.any(steep)
    # TraceLine swaps the ends when the major coordinate falls: both orders beyond the 32-bit path
    falls = np.where(steep, dy, dx) < 0
    assert np.any(falls & (major > 32767)) and np.any(~falls & (major > 32767))
    assert np.any(falls & (major == 32767)) and np.any(~falls & (major == 32767))
    # rays that leave the map (the clipped one) and rays that end on it
    on_map = (rays[:, 2] >= 0) & (rays[:, 2] < e["width"]) & (rays[:, 3] >= 0) & (rays[:, 3] < e["height"])
    assert np.any(on_map) and not np.all(on_map)
    for x0, y0, x1, y1, _ in rays.tolist():
        lit = R.literal_line(x0, y0, x1, y1)
        np.testing.assert_array_equal(R.closed_line(x0, y0, x1, y1), lit, err_msg=str((x0, y0, x1, y1)))
        tiled = R.tiled_line(x0, y0, x1, y1, tile=64)
        np.testing.assert_array_equal(_as_sorted_rows(tiled), _as_sorted_rows(lit), err_msg=str((x0, y0, x1, y1)))


def test_far_ends_case_needs_64_bit_products():
    """case_far_ends: clipped rays of 10^6 cells across a 3401 x 4440 map.  On the map's own cells the closed
    form's numerator 2 * i * deltaY + deltaX exceeds 2^32 (it cannot on any ray of case_long_lines, whose
    2 * 45000^2 < 2^32), in both end orders; and the walk over the map's tiles as kg_trace_kernel makes it
    emits exactly the literal loop's on-map cells."""
    c = R.case_far_ends()
    e = R.create_from_scans(c)
    w, h = e["width"], e["height"]
    assert (w, h) == (3401, 4440) and w * h <= 1 << 24 and e["pass"].sum() > 0 and e["hits"].sum() > 0
    assert c["laser"]["range_threshold"] / c["resolution"] <= 1 << 20       # kg_create's bound on a ray
    rays = R.ray_cells(c, e).reshape(-1, 5)
    rays = rays[rays[:, 4] >= 0]
    assert len(rays) == 14 and np.count_nonzero(rays[:, 4] == 0) == 10       # ten clipped to range_threshold
    assert 2 * 45000 * 45000 + 45000 < 1 << 32                               # the longest ray of case_long_lines
    wide = {False: 0, True: 0}                                               # end order -> rays beyond 32 bits
    for x0, y0, x1, y1, _ in rays.tolist():
        lit = R.literal_line(x0, y0, x1, y1)
        on = lit[(lit[:, 0] >= 0) & (lit[:, 0] < w) & (lit[:, 1] >= 0) & (lit[:, 1] < h)]
        got = R.map_line(x0, y0, x1, y1, w, h)
        assert len(got) == len(on), (x0, y0, x1, y1)
        if len(on):
            np.testing.assert_array_equal(_as_sorted_rows(got), _as_sorted_rows(on), err_msg=str((x0, y0, x1, y1)))
        dx, dy = abs(x1 - x0), abs(y1 - y0)
        steep = dy > dx
        major0, major1 = (y0, y1) if steep else (x0, x1)
        if len(on) > 1000:   # a ray that crosses the map: the major steps (after TraceLine's swaps) of its cells
            i = (on[:, 1] if steep else on[:, 0]).astype(np.int64) - min(major0, major1)
            if 2 * int(i.max()) * min(dx, dy) + max(dx, dy) >= 1 << 32:
                wide[major0 > major1] += 1
    assert wide[False] >= 1 and wide[True] >= 1, wide


@pytest.mark.parametrize("w,h", R.DIMS)
def test_dims_case_gives_the_requested_map(w, h):
    c, e, rc = _built("dims", w, h)
    assert (e["width"], e["height"]) == (w, h) and np.all(c["poses"] == 0) and len(c["poses"]) == 3
    assert e["pass"].sum() > 0 and e["hits"].sum() > 0
    traced = rc[0][rc[0][:, 4] >= 0]
    ox, oy = traced[0, :2]
    assert np.all(traced[:, 0] == ox) and np.all(traced[:, 1] == oy)
    # a single column / row: the scans' own cell lies one past it, the rays along the other axis are off the map
    assert ox == (w if w == 1 else w // 2) and oy == (h if h == 1 else h // 2)
    if w == 1 or h == 1:
        assert e["pass"].sum() == 6 and e["hits"].sum() == 3 and np.count_nonzero(e["pass"]) == 1
        assert len(traced) == 3                              # two of the three rays lie wholly off the map
    else:
        assert e["state"][oy, ox] == 255 and e["pass"][oy, ox] == 12


def test_dims_set_covers_the_plane_and_tile_edges():
    cells = [w * h for w, h in R.DIMS]
    assert {0, 1, 15} <= {n % 16 for n in cells} and any(n < 16 for n in cells)   # kg_update_kernel's groups of 16
    assert any(n == 16 for n in cells)                                              # exactly one full group
    assert any(w % 64 == 0 and h % 64 == 0 for w, h in R.DIMS)                      # the tile clamp is a no-op
    assert any(w % 64 == 1 for w, h in R.DIMS) and any(h % 64 == 1 for w, h in R.DIMS)   # a tile one cell wide / high
    assert any(w % 64 == 63 for w, h in R.DIMS) and any(h % 64 == 63 for w, h in R.DIMS)
    assert any(h == 1 for w, h in R.DIMS) and any(w == 1 for w, h in R.DIMS)
    assert (1, 1) not in R.DIMS                                                     # an all-zero map: vacuous


@pytest.mark.parametrize("n", R.BEAMS)
def test_beams_case(n):
    c, e, rc = _built("beams", n)
    assert c["laser"]["n_readings"] == n == c["ranges"].shape[1] and len(c["poses"]) == 2
    assert np.all(rc[..., 4] == 1) and e["pass"].sum() > 0
    # n = 1: the two ends are the box's own maxima, which round to index == width and == height: no hit on the map
    assert e["hits"].sum() == 0 if n == 1 else e["hits"].sum() > 0
    assert (e["width"], e["height"]) == ((58, 55) if n == 1 else (117, 93))
    assert set(R.BEAMS) >= {1, 64, 256, 257, 4096}     # around the loops' strides of 256, and kg_create's limit


# ------------------------------------------------------------------ the plain float64 model against the restatement
PLAIN_MARGIN = 1e-6   # cells; a last-place difference of sin / cos moves a point by about 1e-11 cells here
PLAIN_CASES = {"rounds600": lambda: R.case_rounds(600), "one67": R.case_one, "rules": R.case_rules,
               "thresholds": R.case_thresholds}
PLAIN_CASES.update({f"dims{w}x{h}": functools.partial(R.case_dims, w, h) for w, h in R.DIMS})
PLAIN_CASES.update({f"beams{n}": functools.partial(R.case_beams, n) for n in R.BEAMS})


@pytest.mark.parametrize("name", list(PLAIN_CASES))
def test_plain_model_equals_restatement(name):
    """tests/ref/karto_grid_plain.py (math.sin / math.cos, written from the reference text) against the
    restatement (detmath.h): provided no traced end point, scan position or map extent of the input lies within
    1e-6 cells of a rounding boundary, the dimensions and all four planes are equal, every cell, and the offset
    agrees within 1e-12 m (a 45 m reading times a last-place cosine error is about 1e-14).

    `rules` is the one input that does not meet the condition, by its own design: beam 20 (120 degrees, 1.15 m)
    ends 7e-15 cells from the boundary 18.5, and beams 13 and 14 read range_threshold and range_threshold - 5e-7
    (threshold margin 0; those comparisons involve no arithmetic).  Its maps are compared all the same."""
    c = PLAIN_CASES[name]()
    p = P.create_from_scans(c)
    e = R.create_from_scans(c)
    print(f"{name}: margin {p['margin']:.3g} cells, threshold margin {p['threshold_margin']:.3g} cells")
    if name == "rules":
        assert p["margin"] < PLAIN_MARGIN and p["threshold_margin"] == 0.0   # see the docstring
    else:
        assert p["margin"] >= PLAIN_MARGIN and p["threshold_margin"] >= PLAIN_MARGIN
    assert (p["width"], p["height"]) == (e["width"], e["height"])
    assert np.abs(p["offset"] - e["offset"]).max() <= 1e-12
    for k in ("pass", "hits", "state", "ros"):
        assert p[k].dtype == e[k].dtype and p[k].shape == e[k].shape
        np.testing.assert_array_equal(p[k], e[k], err_msg=k)
    assert p["pass"].sum() > 0


def test_plain_model_hand_cases():
    """The model's own line and cell rounding against the hand-counted cases above (not against the restatement)."""
    assert P.trace_line(2, 5, 1, 0) == [(1, 0), (1, 1), (1, 2), (2, 3), (2, 4), (2, 5)]
    assert P.trace_line(0, 0, 3, 3) == [(0, 0), (1, 1), (2, 2), (3, 3)]
    assert P.trace_line(3, 2, 3, 2) == [(3, 2)]
    e = P.create_from_scans(R.case_thresholds())
    assert (e["width"], e["height"]) == (70, 70)
    assert (e["pass"][30, 50], e["hits"][30, 50], e["state"][30, 50], e["ros"][30, 50]) == (10, 1, 255, 0)
    assert (e["pass"][50, 30], e["hits"][50, 30], e["state"][50, 30], e["ros"][50, 30]) == (9, 1, 100, 100)
    assert (e["pass"][30, 20], e["state"][30, 20], e["ros"][30, 20]) == (2, 0, -1)
    assert (e["pass"][30, 0], e["hits"][30, 0], e["state"][30, 0]) == (4, 2, 100)
    assert e["pass"][30, 30] == 9 + 8 + 2 + 3
