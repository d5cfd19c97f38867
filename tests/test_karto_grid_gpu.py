"""GPU parity of the Karto occupancy-grid rebuild (karto::OccupancyGrid::CreateFromScans, Karto.h:5659-5673, as
kg_bbox / kg_rays / kg_trace / kg_update kernels) against the CPU restatement tests/ref/karto_grid_ref.c.
Bar: bit-exact -- every cell of pass, hits, state and ros, the width and height and the bits of the offset; no
tolerance and no cell left out (the counters are integers, so the sums are order-free).  The context's planes
are poisoned before a build and read back past the map, so a write out of place shows.  open_karto needs boost
and is not built, so parity with the library itself is unpinned, as for the matcher.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import karto_grid_ref as R  # noqa: E402

from slam2d import karto, karto_grid  # noqa: E402
from slam2d.karto_grid import KgInfo, OccupancyGridBuilder  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = 0xA5
H2D, D2H = 1, 2


@functools.lru_cache(maxsize=None)
def _hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return h


@functools.lru_cache(maxsize=None)
def _want(name):
    """The restatement's map of a named case, computed once and shared (treat as read-only)."""
    c = CASES[name]()
    return c, R.create_from_scans(c)


CASES = {"one67": R.case_one, "cross48": R.case_cross, "same64": R.case_same_pose, "rules": R.case_rules,
         "thresholds": R.case_thresholds, "thresholds_alt": lambda: R.case_thresholds(4, 0.5), "fine": R.case_fine,
         "mini": lambda: R.case_cross(S=6, n=67, seed=7)}


def _laser(lz):
    return karto.laser(lz["n_readings"], lz["minimum_angle"], lz["angular_resolution"], lz["minimum_range"],
                       lz["range_threshold"])


def _params(c):
    p = karto_grid.default_params(c["laser"]["maximum_range"], c["resolution"])
    p.occupancy_threshold = c["occupancy_threshold"]
    p.min_pass_through = c["min_pass_through"]
    return p


def _builder(c, max_scans=None, max_cells=None, want=None):
    cells = max_cells if max_cells is not None else max(want["width"] * want["height"], 1) + 1000
    return OccupancyGridBuilder(_laser(c["laser"]), _params(c), max_scans or len(c["poses"]), cells)


def _poison(b):
    """Fill all four device planes of the context, to their allocated end."""
    cells = (b.max_cells + 15) & ~15
    for k, ptr in b.device_planes().items():
        assert _hip().hipMemset(ptr, POISON, cells * (4 if k in ("pass", "hits") else 1)) == 0


def _planes_with_tail(b):
    """The device planes, whole: [max_cells] per plane."""
    out = {}
    for k, ptr in b.device_planes().items():
        a = np.zeros(b.max_cells, {"state": np.uint8, "ros": np.int8, "pass": np.uint32, "hits": np.uint32}[k])
        assert _hip().hipMemcpy(a.ctypes.data_as(C.c_void_p), ptr, a.nbytes, D2H) == 0
        out[k] = a
    return out


def _check_build(b, c, want):
    """One poisoned build of case c on builder b against `want`, through the host arrays."""
    _poison(b)
    got = b.create_from_scans(c["ranges"], c["poses"])
    R.assert_maps_equal(got, want)
    cells = want["width"] * want["height"]
    for k, a in _planes_with_tail(b).items():
        np.testing.assert_array_equal(a[:cells].reshape(want[k].shape), want[k], err_msg=k)
        tail = a[cells:].view(np.uint8)
        assert np.all(tail == POISON), f"{k} was written past width * height"
    # kg_get_map writes exactly width * height elements of a larger, poisoned host buffer
    st = np.full(cells + 64, POISON, np.uint8)
    ps = np.full(cells + 64, 0xA5A5A5A5, np.uint32)
    assert b.L.kg_get_map(b.h, st.ctypes.data_as(C.c_void_p), None, ps.ctypes.data_as(C.c_void_p), None) == 0
    assert np.all(st[cells:] == POISON) and np.all(ps[cells:] == 0xA5A5A5A5)
    np.testing.assert_array_equal(st[:cells].reshape(want["state"].shape), want["state"])
    return got


@pytest.fixture(params=["auto", "1", "3"])
def split(request, monkeypatch):
    """Workgroups per tile: the library's rule, one owner per tile (plain stores, no memset), three sharing a
    tile's scan list (atomic merge into zeroed planes)."""
    if request.param == "auto":
        monkeypatch.delenv("SLAM2D_KG_SPLIT", raising=False)
    else:
        monkeypatch.setenv("SLAM2D_KG_SPLIT", request.param)
    return request.param


def test_one_scan_67_beams(gpu, split):
    c, want = _want("one67")
    assert len(c["poses"]) == 1 and c["laser"]["n_readings"] % 64 != 0
    b = _builder(c, want=want)
    _check_build(b, c, want)
    b.close()


def test_trajectory_crossing_tiles(gpu, split):
    c, want = _want("cross48")
    w, h = want["width"], want["height"]
    assert w > 128 and h > 128 and w % 8 and h % 8 and w % 64 and h % 64, (w, h)
    assert np.all(c["poses"][:, :2] < 0)
    # rays in all eight octants, exactly axis-aligned and exactly diagonal ones among them (in cells)
    lz, res = c["laser"], c["resolution"]
    s = np.arange(len(c["poses"]))[:, None]
    a = c["poses"][:, 2:3] + lz["minimum_angle"] + np.arange(lz["n_readings"])[None, :] * lz["angular_resolution"]
    ok = (c["ranges"] > lz["minimum_range"]) & (c["ranges"] < lz["range_threshold"] - 1e-3)
    r = np.where(ok, c["ranges"], 0.0)
    to_cell = lambda v, o: np.floor((v - o) / res + 0.5).astype(np.int64)  # noqa: E731
    dx = to_cell(c["poses"][s, 0] + r * np.cos(a), want["offset"][0]) - to_cell(c["poses"][s, 0], want["offset"][0])
    dy = to_cell(c["poses"][s, 1] + r * np.sin(a), want["offset"][1]) - to_cell(c["poses"][s, 1], want["offset"][1])
    dx, dy = dx[ok], dy[ok]
    octants = {(int(x > 0), int(y > 0), int(abs(x) > abs(y))) for x, y in zip(dx, dy) if x and y and abs(x) != abs(y)}
    assert len(octants) == 8
    for sx, sy in [(1, 0), (-1, 0), (0, 1), (0, -1)]:
        assert np.any((np.sign(dx) == sx) & (np.sign(dy) == sy)), "no axis-aligned ray"
    for sx, sy in [(1, 1), (1, -1), (-1, 1), (-1, -1)]:
        assert np.any((np.abs(dx) == np.abs(dy)) & (np.sign(dx) == sx) & (np.sign(dy) == sy)), "no diagonal ray"
    b = _builder(c, want=want)
    _check_build(b, c, want)
    b.close()


def test_64_scans_at_one_pose(gpu, split):
    c, want = _want("same64")
    b = _builder(c, want=want)
    got = _check_build(b, c, want)
    b.close()
    lz = c["laser"]
    traced = int(np.sum(~((c["ranges"] <= lz["minimum_range"]) | (c["ranges"] >= lz["maximum_range"])
                          | np.isnan(c["ranges"]))))
    ox, oy = R.beam_cell(c, want, 0, 0, 0.0)
    assert traced == 64 * lz["n_readings"]
    assert got["pass"][oy, ox] == traced and got["pass"].max() == traced  # the contended cell: one per ray of every scan


def test_reading_rules(gpu, split):
    """NaN, +inf, 0, negative, == minimum_range and == maximum_range are not traced; >= range_threshold is clipped
    (and leaves the box: the scan's other readings are short); [thr - 1e-6, thr) is traced unclipped without a hit;
    just below the band scores the hit.  Each beam is 15 degrees from its neighbours, so 1 m out its cells are its own."""
    c, want = _want("rules")
    b = _builder(c, want=want)
    got = _check_build(b, c, want)
    b.close()
    ps, ht = got["pass"], got["hits"]

    def around(i, r):
        x, y = R.beam_cell(c, want, 0, i, r)
        assert 1 <= x < want["width"] - 1 and 1 <= y < want["height"] - 1
        return int(ps[y - 1:y + 2, x - 1:x + 2].sum())

    for i in (2, 4, 5, 8, 9, 10):   # NaN, +inf, 0, -1, == minimum_range, == maximum_range
        assert around(i, 1.0) == 0, i
    for i in (1, 3, 7, 13, 14, 16, 18):  # clipped (5.0, 6.0, 7.9, == thr), the band, below the band, a long valid one
        assert around(i, 1.0) >= 1, i
    # the clipped beams' ends are off the map on two different sides: the -x side (beam 1) and the -y side (beam 7)
    assert R.beam_cell(c, want, 0, 1, R.RULES_THR)[0] < 0 and R.beam_cell(c, want, 0, 7, R.RULES_THR)[1] < 0
    x, y = R.beam_cell(c, want, 0, 3, R.RULES_THR)
    assert x < 0 and y < 0
    assert around(1, 1.4) >= 1 and around(7, 1.4) >= 1  # and they are traced beyond the other readings' reach
    x, y = R.beam_cell(c, want, 0, 14, R.RULES_READINGS[14])
    assert (ps[y, x], ht[y, x]) == (1, 0)
    x, y = R.beam_cell(c, want, 0, 16, R.RULES_READINGS[16])
    assert (ps[y, x], ht[y, x]) == (2, 1)
    x, y = R.beam_cell(c, want, 0, 13, R.RULES_THR)  # == range_threshold: in the box (its maximum: index == width)
    assert x == want["width"] and ht[y, x - 1] == 0 and ps[y, x - 1] == 1  # ... clipped with ratio 1, no hit
    x, y = R.beam_cell(c, want, 0, 9, R.RULES_MIN)   # == minimum_range is in the bounding box but not traced
    assert ht[y, x] == 0


def test_thresholds(gpu):
    c, want = _want("thresholds")
    b = _builder(c, want=want)
    e = _check_build(b, c, want)
    b.close()
    assert (e["pass"][30, 50], e["hits"][30, 50], e["state"][30, 50], e["ros"][30, 50]) == (10, 1, 255, 0)
    assert (e["pass"][50, 30], e["hits"][50, 30], e["state"][50, 30], e["ros"][50, 30]) == (9, 1, 100, 100)
    assert (e["pass"][30, 20], e["state"][30, 20], e["ros"][30, 20]) == (2, 0, -1)
    assert (e["pass"][20, 30], e["state"][20, 30], e["ros"][20, 30]) == (3, 255, 0)
    c2, want2 = _want("thresholds_alt")
    b = _builder(c2, want=want2)
    e = _check_build(b, c2, want2)
    b.close()
    assert e["state"][20, 30] == 0 and e["state"][50, 30] == 255 and e["state"][30, 0] == 0


def test_golden_cases(gpu):
    for name, (c, want) in R.load_golden().items():
        b = _builder(c, want=want)
        _check_build(b, c, want)
        b.close()


def test_back_to_back_builds(gpu, split):
    """The second build is smaller and shifted: nothing of the first may survive in its planes."""
    c1, _ = _want("cross48")
    c2, w2 = _want("mini")
    n = c2["laser"]["n_readings"]
    c1s = dict(c1, ranges=c1["ranges"][:, :n].copy(), laser=c2["laser"])  # the same laser: one context
    w1s = R.create_from_scans(c1s)
    assert w2["width"] * w2["height"] < w1s["width"] * w1s["height"] and not np.array_equal(w1s["offset"], w2["offset"])
    b = _builder(c1s, want=w1s)
    R.assert_maps_equal(b.create_from_scans(c1s["ranges"], c1s["poses"]), w1s)
    R.assert_maps_equal(b.create_from_scans(c2["ranges"], c2["poses"]), w2)
    R.assert_maps_equal(b.create_from_scans(c1s["ranges"], c1s["poses"]), w1s)
    b.close()


def test_erange_reports_dimensions(gpu):
    c, want = _want("one67")
    b = _builder(c, max_cells=1000)
    with pytest.raises(karto_grid.MapTooLarge) as ei:
        b.create_from_scans(c["ranges"], c["poses"])
    assert (ei.value.width, ei.value.height) == (want["width"], want["height"])
    np.testing.assert_array_equal(ei.value.offset.view(np.int64), want["offset"].view(np.int64))
    assert b.get_map()["pass"].size == 0
    info = KgInfo()
    r, p = np.ascontiguousarray(c["ranges"]), np.ascontiguousarray(c["poses"])
    rc = b.L.kg_build(b.h, 1, r.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), C.byref(info))
    assert rc == karto_grid.KG_ERANGE and info.status == karto_grid.KG_ERANGE and b"max_cells" in b.L.kg_last_error()
    b.close()
    b = _builder(c, max_cells=ei.value.width * ei.value.height)  # exactly enough
    _check_build(b, c, want)
    b.close()


def test_empty_map_and_no_scans(gpu):
    c = R.case_empty()
    want = R.create_from_scans(c)
    assert (want["width"], want["height"]) == (0, 0)
    b = _builder(c, max_cells=100)
    _poison(b)
    got = b.create_from_scans(c["ranges"], c["poses"])
    assert (got["width"], got["height"]) == (0, 0) and got["pass"].size == 0
    np.testing.assert_array_equal(got["offset"].view(np.int64), want["offset"].view(np.int64))
    for k, a in _planes_with_tail(b).items():
        assert np.all(a.view(np.uint8) == POISON), k  # nothing was launched
    info = KgInfo()
    rc = b.L.kg_build(b.h, 0, None, None, C.byref(info))
    assert rc == karto_grid.KG_EINVAL and b"no grid" in b.L.kg_last_error()
    b.close()


def test_create_rejects_bad_parameters(gpu):
    c = R.case_one()
    for res, mx in [(0.0, 30.0), (0.05, 0.0), (-1.0, 30.0)]:
        p = karto_grid.default_params(mx, res)
        with pytest.raises(karto_grid.Slam2dError):
            OccupancyGridBuilder(_laser(c["laser"]), p, 4, 1000)
    p = karto_grid.default_params(0.0)
    assert (p.resolution, p.occupancy_threshold, p.min_pass_through, p.maximum_range) == (0.05, 0.1, 2, 0.0)


def test_pool_path_equals_direct(gpu):
    """The map built from the matcher's pool (kt_pool_device) equals the map built from the same arrays."""
    import torch

    c, want = _want("cross48")
    S = len(c["poses"])
    m = karto.ScanMatcher(_laser(c["laser"]), max_matches=1, max_scans=S + 3, max_base=4)
    m.set_scans(0, c["ranges"], c["poses"])
    d_r, d_p, cap = m.pool_device()
    assert d_r and d_p and cap == S + 3
    b = _builder(c, want=want)
    _poison(b)
    R.assert_maps_equal(b.create_from_scans_device(S, d_r, d_p), want)
    tr = torch.from_numpy(c["ranges"]).cuda()
    tp = torch.from_numpy(c["poses"]).cuda()
    _poison(b)
    hs = torch.cuda.current_stream().cuda_stream
    assert b.create_from_scans_device(S, tr, tp, hip_stream=hs, fetch=False)[:2] == (want["width"], want["height"])
    R.assert_maps_equal(b.get_map(), want)
    times = b.kernel_times()
    assert set(times) >= {"kg_bbox_kernel", "kg_trace_kernel", "kg_update_kernel"}
    b.close()
    m.close()


def test_fine_resolution_long_rays(gpu, split):
    """Resolution 0.01: rays of several hundred major steps, a map of over a hundred tiles."""
    c, want = _want("fine")
    assert c["resolution"] == 0.01 and c["laser"]["n_readings"] == 361 and want["width"] > 640
    b = _builder(c, want=want)
    R.assert_maps_equal(b.create_from_scans(c["ranges"], c["poses"]), want)
    b.close()


# ------------------------------------------------------------------ directed cases (tests/ref/karto_grid_ref.py; that
# each takes the path it is named for is asserted without a GPU in tests/test_karto_grid_cpu.py)
CASES.update({f"rounds{S}": functools.partial(R.case_rounds, S) for S in (257, 513, 600)})
CASES["rounds600_one_pose"] = functools.partial(R.case_rounds, 600, one_pose=True)
CASES.update({f"dims{w}x{h}": functools.partial(R.case_dims, w, h) for w, h in R.DIMS})
CASES.update({f"beams{n}": functools.partial(R.case_beams, n) for n in R.BEAMS})


@functools.lru_cache(maxsize=1)
def _want_long(orientation):
    """The restatement's map of a long-line case; one at a time (13 M cells, 130 MB of planes)."""
    c = R.case_long_lines(orientation)
    return c, R.create_from_scans(c)


def _set_split(monkeypatch, value):
    if value == "auto":
        monkeypatch.delenv("SLAM2D_KG_SPLIT", raising=False)
    else:
        monkeypatch.setenv("SLAM2D_KG_SPLIT", value)
    return value


@pytest.fixture(params=["auto", "1", "2", "3", "32"])
def split5(request, monkeypatch):
    """`split`, and also two parts (more than 256 scans per part at 513 and 600 scans) and the largest split, 32
    (a short last part at 600 scans, empty parts at 513 and 257)."""
    return _set_split(monkeypatch, request.param)


@pytest.fixture(params=["auto", "3"])
def split_auto3(request, monkeypatch):
    return _set_split(monkeypatch, request.param)


@pytest.mark.parametrize("S", [257, 513, 600])
def test_scan_list_rounds(gpu, split5, S):
    """More scans than kg_trace_kernel lists in one round, and than kg_bbox_reduce_kernel takes in one step; the
    map's right-hand tile column is met by scans of the later rounds only."""
    c, want = _want(f"rounds{S}")
    assert len(c["poses"]) == S > 256 and want["width"] > 64 and want["pass"][:, 64:].sum() > 0
    b = _builder(c, want=want)
    _check_build(b, c, want)
    b.close()


def test_600_scans_at_one_pose(gpu, split5):
    c, want = _want("rounds600_one_pose")
    b = _builder(c, want=want)
    got = _check_build(b, c, want)
    b.close()
    ox, oy = R.ray_cells(c, want)[0, 0, :2]
    assert got["pass"][oy, ox] == 600 * c["laser"]["n_readings"] == got["pass"].max()


@pytest.mark.parametrize("order", ["shuffled", "halves_swapped"])
def test_scan_order_invariance(gpu, monkeypatch, order):
    """The planes do not depend on the order of the scans (and so not on which round or part lists a scan):
    device against device, under the library's split rule and with one owner per tile."""
    c, want = _want("rounds600")
    S = len(c["poses"])
    perm = np.random.default_rng(17).permutation(S) if order == "shuffled" else np.r_[256:512, 0:256, 512:S]
    assert sorted(perm.tolist()) == list(range(S)) and perm[0] != 0
    maps = []
    for value in ("auto", "1"):
        _set_split(monkeypatch, value)
        b = _builder(c, want=want)
        _poison(b)
        maps.append(b.create_from_scans(c["ranges"], c["poses"]))
        _poison(b)
        maps.append(b.create_from_scans(c["ranges"][perm], c["poses"][perm]))
        b.close()
    for m in maps[1:]:
        R.assert_maps_equal(m, maps[0])
    assert maps[0]["pass"].sum() > 0


@pytest.mark.parametrize("orientation,value", [("x", "auto"), ("x", "1"), ("x", "3"), ("y", "auto"), ("slant", "auto")])
def test_long_lines_64bit_path(gpu, monkeypatch, orientation, value):
    """Rays of 32767, 32768 and up to 45000 major steps at resolution 0.001: the 64-bit division of
    csrc/karto_grid_line.h's clip, carry and error as device code, in both end orders."""
    _set_split(monkeypatch, value)
    c, want = _want_long(orientation)
    assert want["width"] * want["height"] <= 1 << 24 and max(want["width"], want["height"]) > 40000
    b = _builder(c, want=want)
    _check_build(b, c, want)
    b.close()


@pytest.mark.parametrize("value", ["auto", "3"])
def test_far_ends_64bit_products(gpu, monkeypatch, value):
    """Clipped rays of 10^6 cells (kg_create admits 2^20) across a 3401 x 4440 map: on the map's own cells
    2 * i * deltaY + deltaX exceeds 2^32, which no ray of the long-line cases reaches (2 * 45000^2 < 2^32), so
    only here would a 32-bit division in the device's clip, carry or error show."""
    _set_split(monkeypatch, value)
    c = R.case_far_ends()
    want = R.create_from_scans(c)
    assert (want["width"], want["height"]) == (3401, 4440) and want["hits"].sum() > 0
    b = _builder(c, want=want)
    _check_build(b, c, want)
    b.close()


@pytest.mark.parametrize("w,h", R.DIMS)
def test_map_dimensions(gpu, split_auto3, w, h):
    """Maps of fewer than 16 cells, of exactly one group of 16, of whole tiles, with a tile one cell wide or
    high, single rows and columns (the scans' own cell then lies off the map)."""
    c, want = _want(f"dims{w}x{h}")
    assert (want["width"], want["height"]) == (w, h) and want["pass"].sum() > 0
    b = _builder(c, want=want)
    _check_build(b, c, want)
    b.close()
    b = _builder(c, max_cells=w * h)   # exactly enough: the planes end with the map (rounded up to 16 cells)
    _check_build(b, c, want)
    b.close()


@pytest.mark.parametrize("n", R.BEAMS)
def test_beam_counts(gpu, monkeypatch, n):
    _set_split(monkeypatch, "auto")
    c, want = _want(f"beams{n}")
    assert c["laser"]["n_readings"] == n
    b = _builder(c, want=want)
    _check_build(b, c, want)
    b.close()


def test_back_to_back_600_5_600(gpu, split):
    """One context for 600 scans: 600, then the first 5 of them, then the 600 again.  Nothing of the larger
    build's scan records, ray words or planes may survive into the smaller one."""
    c, want = _want("rounds600")
    c5 = dict(c, ranges=c["ranges"][:5].copy(), poses=c["poses"][:5].copy())
    want5 = R.create_from_scans(c5)
    assert 0 < want5["width"] * want5["height"] < want["width"] * want["height"]
    b = _builder(c, max_scans=600, want=want)
    _check_build(b, c, want)
    _check_build(b, c5, want5)
    _check_build(b, c, want)
    b.close()
