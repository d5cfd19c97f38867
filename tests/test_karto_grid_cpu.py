"""The Karto occupancy-grid rebuild without a GPU: the CPU restatement tests/ref/karto_grid_ref.c against its golden
file and against counts typed out by hand from Grid::TraceLine / OccupancyGrid::RayTrace (Karto.h:4680-4745,
:5910-5945), and the closed form of csrc/karto_grid_line.h (what kg_trace_kernel walks) against the literal loop.
open_karto needs boost and is not built here; the hand-written cases pin the restatement to the reference text.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
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
