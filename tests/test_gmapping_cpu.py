"""GMapping single-scan grid (config 4) -- the oracle against the REFERENCE.

The reference's GMapping grid headers (lesson4/include/lesson4/gmapping/grid/*.h) compile
unmodified; oracle/Makefile builds them into oracle/_ref/libgmapping_ref.so (container only) and
oracle/make_golden.py stored their outputs in tests/golden/gmapping_ref.npz.  The C restatement
(oracle/gmapping_oracle.c) must reproduce them bit for bit: integer (n, visits) counts and the
float PointAccumulator sums.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import gmapping_cases as G  # noqa: E402
import gmapping_model as M  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                      "libgmapping_ref.so")


def _sparse(n, v, acc):
    idx = np.nonzero(v.ravel())[0].astype(np.int32)
    return idx, n.ravel()[idx], v.ravel()[idx], acc.reshape(-1, 2)[idx].view(np.int32)


def test_geometry():
    """ScanMatcherMap(Point(0,0), -40,-40,40,40, 0.05): 1600 x 1600, world2map(0,0) = (800,800)
    (SURVEY.md §8c probe)."""
    sx, sy, sx2, sy2 = O.gm_geometry()
    assert (sx, sy, sx2, sy2) == (1600, 1600, 800, 800)


@pytest.mark.parametrize("i", range(4))
def test_oracle_matches_reference_fixture(i):
    d = np.load(os.path.join(GOLD, "gmapping_ref.npz"))
    ang = d["angles"]
    x, y, c, s = (float(v) for v in d[f"p{i}_pose"])
    n, v, acc, nfree, nhits = O.gm_compute(d[f"p{i}_ranges"], np.cos(ang), np.sin(ang), (x, y, c, s))
    idx, nn, vv, ab = _sparse(n, v, acc)
    np.testing.assert_array_equal(idx, d[f"p{i}_idx"])
    np.testing.assert_array_equal(nn, d[f"p{i}_n"])
    np.testing.assert_array_equal(vv, d[f"p{i}_visits"])
    np.testing.assert_array_equal(ab, d[f"p{i}_acc_bits"])
    assert [nfree, nhits] == list(d[f"p{i}_counts"])


def test_fixture_edge_cases_present():
    """The fixture exercises d == 0, d > max_urange (clamped, no hit), d > max_range, inf."""
    d = np.load(os.path.join(GOLD, "gmapping_ref.npz"))
    r = d["p0_ranges"]
    assert (r == 0).any() and (r == 27.0).any() and (r == 35.0).any() and np.isinf(r).any()


def _same_maps(a, b):
    for u, w in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(u.view(np.int32) if u.dtype == np.float32 else u,
                                      w.view(np.int32) if w.dtype == np.float32 else w)
    assert a[3:] == b[3:]


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built (needs /root/reference)")
def test_oracle_matches_reference_live():
    """Random poses with theta != 0 and random ranges: oracle == reference build, every cell."""
    rng = np.random.default_rng(3)
    ang = np.linspace(-2.35619449, 2.35619449, 1081)
    for _ in range(6):
        x, y, th = rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(-np.pi, np.pi)
        r = rng.uniform(0.0, 32.0, 1081).astype(np.float32)
        pose = (x, y, np.cos(th), np.sin(th))
        a = O.gm_compute(r, np.cos(ang), np.sin(ang), pose, which="oracle")
        b = O.gm_compute(r, np.cos(ang), np.sin(ang), pose, which="ref")
        _same_maps(a, b)


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("gname", ["small_offset", "fine_long"])
def test_oracle_matches_reference_live_geometries(gname):
    """The off-centre 96 x 64 map and the 4096 x 1024 map at 5 mm (lines of up to 3995 cells, every one inside the
    map: the reference asserts on cells outside it): oracle == reference build, every cell; and the map sizes."""
    p = G.GEOMS[gname]
    sx, sy = C.c_int(), C.c_int()
    O.gmapping_ref_lib().gmr_map_size(p["xmin"], p["ymin"], p["xmax"], p["ymax"], p["delta"], C.byref(sx), C.byref(sy))
    assert (sx.value, sy.value) == G.dims(p)[:2]
    for k in range(2):
        c = G.in_map_beams(gname, k)
        st = c.steps[0]
        a = O.gm_compute(st.ranges, c.a_cos, c.a_sin, tuple(st.poses4[0]), which="oracle", p=p)
        b = O.gm_compute(st.ranges, c.a_cos, c.a_sin, tuple(st.poses4[0]), which="ref", p=p)
        _same_maps(a, b)
        np.testing.assert_array_equal(a[0], c.intended_n(0, 0))


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built (needs /root/reference)")
def test_grid_line_matches_reference():
    """GridLineTraversal::gridLine (gridlinetraversal.h:27-207) incl. the reversal to start at p0: lines of up to
    600 cells as the default geometry draws them, and of up to 6000 cells (max_range / delta at 5 mm)."""
    go, gr = O.gmapping_oracle_lib(), O.gmapping_ref_lib()
    rng = np.random.default_rng(11)
    cap = 6001
    buf_a = np.zeros(2 * cap, np.int32)
    buf_b = np.zeros(2 * cap, np.int32)
    for span, count in ((600, 2000), (6000, 300)):
        for _ in range(count):
            x0, y0 = (int(v) for v in rng.integers(0, 1600, 2))
            x1, y1 = x0 + int(rng.integers(-span, span + 1)), y0 + int(rng.integers(-span, span + 1))
            na = go.gmo_grid_line(x0, y0, x1, y1, O._fp(buf_a))
            nb = gr.gmr_grid_line(x0, y0, x1, y1, O._fp(buf_b), cap)
            assert na == nb == max(abs(x1 - x0), abs(y1 - y0)) + 1
            np.testing.assert_array_equal(buf_a[: 2 * na], buf_b[: 2 * nb])


GEOM_KEYS = [f"{g}{k}" for g in ("small_offset", "fine_long") for k in range(2)]


@pytest.mark.parametrize("key", GEOM_KEYS)
def test_oracle_matches_reference_geometry_fixture(key):
    """tests/golden/gmapping_ref_geom.npz: the reference build's outputs at the two other geometries (directed and
    random beams inside the map, lines of up to 3995 cells), so the pin holds where oracle/_ref is absent."""
    d = np.load(os.path.join(GOLD, "gmapping_ref_geom.npz"))
    p = G.GEOMS[key[:-1]]
    n, v, acc, nfree, nhits = O.gm_compute(d[f"{key}_ranges"], d[f"{key}_a_cos"], d[f"{key}_a_sin"],
                                           tuple(float(x) for x in d[f"{key}_pose"]), p=p)
    idx, nn, vv, ab = _sparse(n, v, acc)
    np.testing.assert_array_equal(idx, d[f"{key}_idx"])
    np.testing.assert_array_equal(nn, d[f"{key}_n"])
    np.testing.assert_array_equal(vv, d[f"{key}_visits"])
    np.testing.assert_array_equal(ab, d[f"{key}_acc_bits"])
    assert [nfree, nhits] == list(d[f"{key}_counts"])
    # the fixture's inputs are the builder's
    c = G.in_map_beams(key[:-1], int(key[-1]))
    np.testing.assert_array_equal(c.a_cos.view(np.int64), d[f"{key}_a_cos"].view(np.int64))
    np.testing.assert_array_equal(c.steps[0].ranges.view(np.int32), d[f"{key}_ranges"].view(np.int32))
    if key.startswith("fine_long"):
        assert np.abs(c.offsets).max() == 3995


def test_small_map_long_beam_stays_in_its_buffer():
    """A 96 x 64-cell map and one 20 m beam: 400 points, more than a buffer sized from the map held (the stand-alone
    sanitizer check of this is `make -C oracle asan-check`).  48 free cells in the map, the rest outside."""
    p = dict(G.GEOMS["small_offset"], xmin=-2.4, xmax=2.4, ymin=-1.6, ymax=1.6)
    n, v, acc, nfree, nhits = O.gm_compute(np.asarray([20.0], np.float32), [1.0], [0.0], p=p)
    assert (nfree, nhits, int(v.sum()), int(n.sum())) == (48, 1, 48, 0)
    assert (v[32, 48:] == 1).all()


# ------------------------------------------------------------------ the case builder (tests/ref/gmapping_cases.py)
def test_geometries():
    assert G.dims(G.GEOMS["small_offset"])[:4] == (96, 64, 48, 32)
    assert G.dims(G.GEOMS["fine_long"])[:4] == (4096, 1024, 2048, 512)
    assert G.GEOMS["fine_long"]["max_range"] / G.GEOMS["fine_long"]["delta"] > 5990


@pytest.mark.parametrize("name", list(G.BUILDERS))
def test_case_ends_are_the_intended_cells(name):
    """From the oracle alone: its hit cells, with their counts, are the cells the case directs its hit beams to."""
    G.check_intent(name)
    c = G.case(name)
    assert len(c.steps[0].poses4) <= 5 and c.a_cos.shape == c.a_sin.shape == (len(c.offsets),)


def test_octant_case_covers_every_direction():
    c = G.case("octants_default")
    offs = {tuple(o) for o in c.offsets}
    for a, b in [(7, 0), (7, 7), (7, 3), (70, 69), (130, 1), (1, 0)]:
        for sa in (1, -1):
            for sb in (1, -1):
                assert (sa * a, sb * b) in offs and (sb * b, sa * a) in offs
    assert (0, 0) in offs
    st = c.steps[0]
    # each end once as a hit and once as a miss; p0 on a tile's last row and column, and on its first
    assert (c.offsets[0::2] == c.offsets[1::2]).all() and st.hit[0::2].all() and not st.hit[1::2].any()
    assert [tuple(v % (G.TILE_W, G.TILE_H)) for v in st.p0] == [(63, 31), (0, 0)]
    n, v = G.oracle_maps("octants_default")[0][0][:2]
    x0, y0 = st.p0[0]
    assert n[y0, x0] == 1 and v[y0, x0] == 1 + (len(offs) - 1) * 2   # the zero-length hit; every other line starts here


def test_multi_hit_case_is_order_sensitive():
    c = G.case("multi_hit")
    n, v, acc = G.oracle_maps("multi_hit")[0][0][:3]
    for cell, beams in ((G.MULTI_C1, G.MULTI_C1_BEAMS), (G.MULTI_C2, G.MULTI_C2_BEAMS)):
        pts = G.hit_points(c, 0, 0, beams)
        assert len({tuple(q) for q in pts.tolist()}) == len(beams)
        assert G.order_sensitive(pts)
        s = np.zeros(2, np.float32)
        for q in pts:
            s = (s + q).astype(np.float32)
        assert n[cell[1], cell[0]] == len(beams)
        np.testing.assert_array_equal(acc[cell[1], cell[0]].view(np.int32), s.view(np.int32))
    b = np.asarray(G.MULTI_C1_BEAMS)
    assert len(set(b // 64)) == 4 and len(set(b // 64 % 4)) >= 3     # fan groups and waves
    assert not c.steps[0].hit[G.MULTI_C1_MISS] and min(b) < G.MULTI_C1_MISS < max(b)
    assert v[G.MULTI_C1[1], G.MULTI_C1[0]] >= len(b)


@pytest.mark.parametrize("rising", [True, False])
def test_tile_sequence_case_pattern(rising):
    name = f"tile_seq_{'rising' if rising else 'falling'}"
    c = G.case(name)
    ntx, nty = G.TSEQ_BOX
    for k in range(2):
        n = G.oracle_maps(name)[0][k][0]
        ys, xs = np.nonzero(n)
        assert len(xs) == ntx * nty and (n[ys, xs] == 1).all()
        assert ((xs % G.TILE_W == G.TSEQ_OFF[0]) & (ys % G.TILE_H == G.TSEQ_OFF[1])).all()
        tiles = (ys // G.TILE_H - G.TSEQ_T0[1]) * ntx + xs // G.TILE_W - G.TSEQ_T0[0]
        assert sorted(tiles) == list(range(ntx * nty))
    # particle 0: the hitting beam's index rises (falls) with the tile index, 70 beams apart
    st = c.steps[0]
    beams = np.nonzero(st.hit)[0]
    e = c.hit_ends(0, 0)
    t = (e[:, 1] // G.TILE_H - G.TSEQ_T0[1]) * ntx + e[:, 0] // G.TILE_W - G.TSEQ_T0[0]
    assert (np.diff(beams) == 70).all() and (np.diff(t) == (1 if rising else -1)).all()


def test_tile_alternating_case_pattern():
    """In box order: marked and unmarked tiles alternate, with one hit tile and free-only tiles; the second step
    turns the hit tile free-only and the other corner into the hit tile."""
    m = G.oracle_maps("tile_alternating")
    k0 = G.tile_kinds(m[0][0][0], m[0][0][1])
    k1 = G.tile_kinds(m[1][0][0], m[1][0][1], box=(10, 20, 12, 22))
    assert k0 == ["f..", "ff.", ".fh"], k0
    assert k1 == ["h..", "ff.", ".ff"], k1


def test_threshold_case_counts():
    n, v = G.oracle_maps("threshold")[0][0][:2]
    (xx, xy), (yx, yy) = G.THRESH_X, G.THRESH_Y
    assert (n[xy, xx], v[xy, xx], n[yy, yx], v[yy, yx]) == (1, 4, 2, 4)
    c = G.case("threshold")
    assert [tuple(e[0]) for e in (c.hit_ends(1, 0), c.hit_ends(1, 1))] == [G.THRESH_X, G.THRESH_Y]


def test_stale_tiles_case_boxes_are_disjoint():
    m = G.oracle_maps("stale_tiles")
    a, b = np.nonzero(m[0][0][1]), np.nonzero(m[0][1][1])
    assert a[0].max() // G.TILE_H < b[0].min() // G.TILE_H and a[1].max() // G.TILE_W < b[1].min() // G.TILE_W
    # the last step marks a few tiles of the box it shares with the step before
    k = G.tile_kinds(m[4][0][0], m[4][0][1])
    assert sum(r.count(".") for r in k) > len(k) and G.tile_kinds(m[3][0][0], m[3][0][1])[1].count(".") == 0


def test_range_edges_case():
    c = G.case("range_edges")
    st = c.steps[0]
    at = np.arange(len(G.EDGE_NAMES)) * 3 + 1
    valid, hit, _, _ = G.end_cells(c.p, st.poses4[0], st.ranges, c.a_cos, c.a_sin)
    got = {nm: (bool(valid[b]), bool(hit[b])) for nm, b in zip(G.EDGE_NAMES, at)}
    assert got == {"0": (False, False), "-0": (False, False), "nan": (False, False), "+inf": (False, False),
                   "-inf": (False, False), "max_range": (True, False), "above_max_range": (False, False),
                   "max_urange": (True, False), "below_max_urange": (True, True), "-3": (True, True)}
    # the oracle agrees beam by beam: each special beam alone
    for nm, b in zip(G.EDGE_NAMES, at):
        r = np.zeros(len(st.ranges), np.float32)
        r[b] = st.ranges[b]
        n, v, _, nfree, nh = O.gm_compute(r, c.a_cos, c.a_sin, tuple(st.poses4[0]), p=c.p)
        assert (nh == 1) == got[nm][1] and (v.sum() > 0) == got[nm][0], nm
        if got[nm][1]:
            x, y = st.p0[0] + c.offsets[b]
            assert n[y, x] == 1


# ------------------------------------------------------------------ the exact-integer model of the kernel's raster
def _grid_line_free(x0, y0, x1, y1, sx, sy, buf):
    k = O.gmapping_oracle_lib().gmo_grid_line(x0, y0, x1, y1, O._fp(buf))
    pts = buf[: 2 * k].reshape(-1, 2)[:-1].astype(np.int64)       # all but p1 (gmapping.cc:227-234)
    assert k == 1 or (pts[0] == (x0, y0)).all()
    return pts[(pts[:, 0] >= 0) & (pts[:, 0] < sx) & (pts[:, 1] >= 0) & (pts[:, 1] < sy)]


def _same_cells(a, b):
    key = lambda c: np.sort(c[:, 1] * (1 << 20) + c[:, 0])        # noqa: E731  (a line visits a cell once)
    return np.array_equal(key(a), key(b))


def test_model_matches_grid_line_random():
    """gm_line / gm_clip / q(i) in exact integers == GridLineTraversal::gridLine on 20000 random lines of up to 600
    cells, clipped per 64 x 32 tile to a 480 x 208-cell map (a 32-cell last tile column, a 16-row last tile row)."""
    rng = np.random.default_rng(2)
    sx, sy = 480, 208
    buf = np.zeros(2 * 700, np.int32)
    for _ in range(20000):
        x0, y0 = int(rng.integers(0, sx)), int(rng.integers(0, sy))
        span = int(rng.choice([3, 40, 600]))
        x1, y1 = x0 + int(rng.integers(-span, span + 1)), y0 + int(rng.integers(-span, span + 1))
        assert _same_cells(M.free_cells(x0, y0, x1, y1, sx, sy), _grid_line_free(x0, y0, x1, y1, sx, sy, buf)), \
            (x0, y0, x1, y1)


def test_steep_entering_case_divides_rounded_numerators():
    """steep_entering: model == gridLine on every line, and in tiles that a line crosses the clip divides numerators
    above 2^24 of the form k d - 1 (they round up to k d as floats): there a float quotient estimate is one too
    high and gm_udiv's downward correction has to run."""
    c = G.case("steep_entering")
    sx, sy = G.dims(c.p)[:2]
    st = c.steps[0]
    buf = np.zeros(2 * 6200, np.int32)
    events = 0
    for k in range(2):
        total = 0
        for off in c.offsets:
            nums = []
            x0, y0 = (int(q) for q in st.p0[k])
            x1, y1 = x0 + int(off[0]), y0 + int(off[1])
            cells = M.free_cells(x0, y0, x1, y1, sx, sy, nums)
            assert _same_cells(cells, _grid_line_free(x0, y0, x1, y1, sx, sy, buf)), (x0, y0, x1, y1)
            total += len(cells)
            two_db = 2 * abs(int(off[0]))
            events += sum(1 for y, crossed in nums if crossed and y > 2 ** 24 and (y + 1) % two_db == 0
                          and float(np.float32(y)) == y + 1)
        assert total == G.oracle_maps("steep_entering")[0][k][3]
    assert events >= 100


def test_model_matches_grid_line_on_long_lines():
    """The long_lines case, line by line: the model's cells are gridLine's, and their number is the oracle's free
    count.  Some clip numerators exceed 2^24 (a float no longer holds them exactly), the largest where the line
    misses the tile and the quotient only has to be large; inside tiles that the line crosses they pass 2^22, where
    a float quotient estimate can be one too high."""
    c = G.case("long_lines")
    sx, sy = G.dims(c.p)[:2]
    buf = np.zeros(2 * 6200, np.int32)
    nums = []
    for s, st in enumerate(c.steps):
        for k in range(len(st.poses4)):
            total = 0
            valid = st.ranges != 0
            for off in c.offsets[: len(st.ranges)][valid]:
                x0, y0 = (int(q) for q in st.p0[k])
                x1, y1 = (int(q) for q in st.p0[k] + (-off if st.flip[k] else off))
                cells = M.free_cells(x0, y0, x1, y1, sx, sy, nums if (s, k) == (0, 0) else None)
                assert _same_cells(cells, _grid_line_free(x0, y0, x1, y1, sx, sy, buf)), (x0, y0, x1, y1)
                total += len(cells)
            assert total == G.oracle_maps("long_lines")[s][k][3]
    nums = np.asarray(nums)
    assert nums[:, 0].max() > 2 ** 24
    assert nums[nums[:, 1] == 1, 0].max() > 2 ** 22
    assert np.abs(c.offsets).max(axis=1).max() > 4000 and (np.abs(c.offsets).max(axis=1) < 5998).all()
